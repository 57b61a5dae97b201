"""Text aligner training timing at B = 2 x 800 mel frames (L = 400) x 150 tokens, fp32 (the shape of
tools/bench_aligner.py): asr.ASRCNN(trainable=True) in train mode on the HIP path, forward, backward and total, split
into the conv stack (MFCC ... projection, ctc_linear) and the S2S decoder; the same module restated in plain
torch-ROCm ops under autograd on the same device in the same session (the conv stack below, tests/s2s_ref.py for the
decoder); and the GroupNorm forward + backward against F.group_norm at [2, 256, 400] for G = 8 and G = 1.  Also the
per-tensor gradient errors of both against the restatement in fp64, all three with the same injected dropout masks.

    python tools/bench_aligner_train.py [out_dir]   -> profiles/aligner_train_bench.json, aligner_train_dtype_err.txt

Warm-up, then the median of 20 timed calls with max - min, hipEvents on the launch stream."""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "styletts2-lite_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from stts2_mi355x import synth  # noqa: E402
from stts2_mi355x import training as Tr  # noqa: E402
from stts2_mi355x.asr import ASRCNN  # noqa: E402

B, T_MEL, L, T_TEXT, N_TOKEN, EMB, REPS, WARM = 2, 800, 400, 150, 178, 512, 20, 3


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": float(np.median(ms)), "spread_ms": float(max(ms) - min(ms))}


class Masks:
    """The keep masks of the 36 ConvBlock dropouts ([B, 256, L]) and of the decoder's one call, on the device."""

    def __init__(self):
        self.m = [torch.from_numpy(synth.dropout_mask(k, (B, 256, L), 0.2)).cuda() for k in range(36)]
        self.m.append(torch.from_numpy(synth.dropout_mask(36, (B, T_TEXT + 1, 128), 0.5)).cuda())

    def __call__(self, k, shape, p):
        return self.m[k]


def torch_features(sd, mel, masks, dt):
    """The conv stack in plain torch ops, channels first as the reference holds it; sd: {name: tensor of dt}."""
    x = torch.matmul(mel.to(dt).transpose(1, 2), sd["to_mfcc.dct_mat"]).transpose(1, 2)
    x = F.conv1d(x, sd["init_cnn.conv.weight"], sd["init_cnn.conv.bias"], stride=2, padding=3)
    k = 0
    for i in range(6):
        for j in range(3):
            p = f"cnns.{i}.0.blocks.{j}."
            h = F.relu(F.conv1d(x, sd[p + "0.conv.weight"], sd[p + "0.conv.bias"], padding=3 ** j, dilation=3 ** j))
            h = F.group_norm(h, 8, sd[p + "2.weight"], sd[p + "2.bias"], 1e-5) * masks.m[k].to(dt) / 0.8
            h = F.relu(F.conv1d(h, sd[p + "4.conv.weight"], sd[p + "4.conv.bias"], padding=1)) * masks.m[k + 1].to(dt) / 0.8
            x = x + h
            k += 2
        x = F.group_norm(x, 1, sd[f"cnns.{i}.1.weight"], sd[f"cnns.{i}.1.bias"], 1e-5)
    return F.conv1d(x, sd["projection.conv.weight"], sd["projection.conv.bias"]).transpose(1, 2)


def torch_ctc(sd, feat):
    h = F.relu(F.linear(feat, sd["ctc_linear.0.linear_layer.weight"], sd["ctc_linear.0.linear_layer.bias"]))
    return F.linear(h, sd["ctc_linear.2.linear_layer.weight"], sd["ctc_linear.2.linear_layer.bias"])


def main():
    from helpers import fill_module
    from s2s_ref import KEYS, s2s_forward
    net = fill_module(ASRCNN(n_token=N_TOKEN, token_embedding_dim=EMB, trainable=True), "asr.").cuda().train()
    mel = np.stack([synth.normal(f"atb:mel:{b}", (80, T_MEL)) for b in range(B)])
    mel[1, :, T_MEL - 40:] = 0.0
    mel = torch.from_numpy(mel).cuda()
    tok = torch.from_numpy(4 + (synth.hash_u01("atb:tok", B * T_TEXT) * 174).astype(np.int64)).view(B, -1).cuda()
    unk = torch.from_numpy(synth.hash_u01("atb:unk", B * T_TEXT) < 0.1).view(B, -1)
    unk_dev = unk.cuda()
    mask = (torch.arange(L)[None, :] >= torch.tensor([L, L - 20])[:, None]).cuda()
    probes = [torch.from_numpy(synth.normal(f"atb:probe:{k}", shp)).cuda() for k, shp in
              (("c", (B, L, N_TOKEN)), ("l", (B, T_TEXT + 1, N_TOKEN)), ("a", (B, T_TEXT + 1, L)))]
    masks = Masks()
    names = [k for k, _ in net.named_parameters()]
    cnn_params = [p for k, p in net.named_parameters() if not k.startswith("asr_s2s.")]
    s2s_params = list(net.asr_s2s.parameters())

    def sd_of(dt):
        sd = {k: p.detach().to(dt).requires_grad_(True) for k, p in net.named_parameters()}
        sd["to_mfcc.dct_mat"] = net.to_mfcc.dct_mat.to(dt)
        return sd

    def hip_all():
        Tr.set_dropout_masks(masks)
        try:
            return net(mel, mask, tok, unk_mask=unk)
        finally:
            Tr.set_dropout_masks(None)

    def hip_cnn():
        Tr.set_dropout_masks(masks)
        try:
            feat = net._features(mel)
            return feat, net._ctc(feat)
        finally:
            Tr.set_dropout_masks(None)

    def hip_s2s(feat):
        Tr.set_dropout_masks(lambda k, shape, p: masks.m[36])
        try:
            return net.asr_s2s(feat, mask, tok, unk_mask=unk)
        finally:
            Tr.set_dropout_masks(None)

    def torch_all(sd, dt):
        feat = torch_features(sd, mel, masks, dt)
        ps = [sd["asr_s2s." + k] for k in KEYS]
        _, logit, attn = s2s_forward(ps, feat, mask, tok, unk_dev, drop_scale=masks.m[36].to(dt) / 0.5)
        return torch_ctc(sd, feat), logit, attn

    def loss_of(o):
        return sum((a * p.to(a.dtype)).sum() for a, p in zip(o, probes))

    out = {"B": B, "T_mel": T_MEL, "L": L, "T_text": T_TEXT, "reps": REPS}
    # ---- the HIP path: total, then the two halves
    out["hip_forward"] = timed(hip_all)
    o = hip_all()
    ls = loss_of(o)
    out["hip_backward"] = timed(lambda: torch.autograd.grad(ls, list(net.parameters()), retain_graph=True))
    out["hip_total"] = timed(lambda: torch.autograd.grad(loss_of(hip_all()), list(net.parameters())))
    out["hip_cnn_forward"] = timed(hip_cnn)
    feat, ctc = hip_cnn()
    pf = torch.from_numpy(synth.normal("atb:probe:f", (B, L, 128))).cuda()
    lc = (feat * pf).sum() + (ctc * probes[0]).sum()
    out["hip_cnn_backward"] = timed(lambda: torch.autograd.grad(lc, cnn_params, retain_graph=True))
    fd = feat.detach().requires_grad_(True)
    out["hip_s2s_forward"] = timed(lambda: hip_s2s(fd))
    so = hip_s2s(fd)
    l2 = (so[1] * probes[1]).sum() + (so[2] * probes[2]).sum()
    out["hip_s2s_backward"] = timed(lambda: torch.autograd.grad(l2, [fd, *s2s_params], retain_graph=True))
    # ---- plain torch-ROCm ops, fp32
    sd32 = sd_of(torch.float32)
    p32 = [sd32[k] for k in names]
    out["torch_forward"] = timed(lambda: torch_all(sd32, torch.float32))
    out["torch_total"] = timed(lambda: torch.autograd.grad(loss_of(torch_all(sd32, torch.float32)), p32))
    out["torch_cnn_forward"] = timed(lambda: torch_features(sd32, mel, masks, torch.float32))
    c32 = [sd32[k] for k in names if not k.startswith(("asr_s2s.", "ctc_linear."))]
    out["torch_cnn_total"] = timed(lambda: torch.autograd.grad(
        (torch_features(sd32, mel, masks, torch.float32) * pf).sum(), c32))
    out["speedup_total"] = out["torch_total"]["median_ms"] / out["hip_total"]["median_ms"]
    # ---- GroupNorm alone at [2, 256, 400]
    for G in (8, 1):
        x = torch.from_numpy(synth.normal(f"atb:gn:{G}", (B, L, 256))).cuda().requires_grad_(True)
        w = torch.ones(256, device="cuda", requires_grad=True)
        b_ = torch.zeros(256, device="cuda", requires_grad=True)
        gy = torch.from_numpy(synth.normal("atb:gn:gy", (B, L, 256))).cuda()
        xt, gyt = x.detach().transpose(1, 2).contiguous().requires_grad_(True), gy.transpose(1, 2).contiguous()
        out[f"groupnorm_G{G}_hip_fwd_bwd"] = timed(
            lambda: torch.autograd.grad(Tr.group_norm_frames(x, w, b_, G), [x, w, b_], gy))
        out[f"groupnorm_G{G}_torch_fwd_bwd"] = timed(
            lambda: torch.autograd.grad(F.group_norm(xt, G, w, b_, 1e-5), [xt, w, b_], gyt))
    # ---- gradient errors against the restatement in fp64
    sd64 = sd_of(torch.float64)
    g64 = torch.autograd.grad(loss_of(torch_all(sd64, torch.float64)), [sd64[k] for k in names])
    g32 = torch.autograd.grad(loss_of(torch_all(sd32, torch.float32)), p32)
    gh = torch.autograd.grad(loss_of(hip_all()), list(net.parameters()))
    gm = max(float(a.abs().max()) for a in g64)
    lines = ["tensor  max|g64|  HIP fp32 vs fp64  torch fp32 vs fp64   (both relative to max(the tensor's max, 1e-3 x "
             "the module's max))"]
    for k, a, h, c in zip(names, g64, gh, g32):
        s = max(float(a.abs().max()), 1e-3 * gm)
        lines.append(f"{k}  {float(a.abs().max()):.3e}  {float((h.double() - a).abs().max()) / s:.2e}  "
                     f"{float((c.double() - a).abs().max()) / s:.2e}")
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles")  # (an output directory may be given)
    os.makedirs(dst, exist_ok=True)
    with open(os.path.join(dst, "aligner_train_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
    with open(os.path.join(dst, "aligner_train_dtype_err.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps(out))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
