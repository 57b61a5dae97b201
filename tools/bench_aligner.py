"""Text aligner timing: ASRCNN.forward + mask_from_lens + maximum_path (train.py:203-214) on the HIP path, with the
split into the conv stack (a forward without tokens), the S2S decoder (the rest of the forward: hoisted products + the
persistent loop) and the search, against the same forward through plain torch-ROCm ops on the drop-in's own
parameters (a restatement written here: one LSTMCell and one attention step per token, as the reference runs it).

    python tools/bench_aligner.py            -> profiles/aligner_bench.json

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
from stts2_mi355x.align import mask_from_lens, maximum_path  # noqa: E402
from stts2_mi355x.asr import ASRCNN  # noqa: E402

T_MEL, T_TEXT, REPS, WARM = 800, 150, 20, 3


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


def eager_forward(net, x, mask, tokens, unk):
    """Modules/ASR/models.py:37-48, 118-176 in torch ops (eval mode)."""
    h = torch.matmul(x.transpose(1, 2), net.to_mfcc.dct_mat).transpose(1, 2)
    c = net.init_cnn.conv
    h = F.conv1d(h, c.weight, c.bias, stride=2, padding=3)
    for layer in net.cnns:
        for blk in layer[0].blocks:
            r = h
            c1, gn, c2 = blk[0].conv, blk[2], blk[4].conv
            h = F.group_norm(F.relu(F.conv1d(h, c1.weight, c1.bias, padding=c1.padding, dilation=c1.dilation)), 8,
                             gn.weight, gn.bias)
            h = F.relu(F.conv1d(h, c2.weight, c2.bias, padding=1)) + r
        h = F.group_norm(h, 1, layer[1].weight, layer[1].bias)
    mem = F.conv1d(h, net.projection.conv.weight, net.projection.conv.bias).transpose(1, 2)
    ctc = net.ctc_linear[2].linear_layer(F.relu(net.ctc_linear[0].linear_layer(mem)))
    s, a = net.asr_s2s, net.asr_s2s.attention_layer
    B, L, D = mem.shape
    hid = cell = ctx = mem.new_zeros(B, D)
    w = cum = mem.new_zeros(B, L)
    pm = a.memory_layer.linear_layer(mem)
    emb = s.embedding(tokens.masked_fill(unk, 3)).transpose(0, 1)
    emb = torch.cat([s.embedding(torch.full((B,), 1, device=x.device)).unsqueeze(0), emb])
    rnn, loc = s.decoder_rnn, a.location_layer
    logits, aligns = [], []
    for e in emb:
        g = F.linear(torch.cat([e, ctx], -1), rnn.weight_ih, rnn.bias_ih) + F.linear(hid, rnn.weight_hh, rnn.bias_hh)
        i, f, gg, o = g.chunk(4, 1)
        cell = torch.sigmoid(f) * cell + torch.sigmoid(i) * torch.tanh(gg)
        hid = torch.sigmoid(o) * torch.tanh(cell)
        pa = loc.location_dense.linear_layer(
            F.conv1d(torch.stack([w, cum], 1), loc.location_conv.conv.weight, padding=31).transpose(1, 2))
        en = a.v.linear_layer(torch.tanh(a.query_layer.linear_layer(hid.unsqueeze(1)) + pa + pm)).squeeze(-1)
        if mask is not None:
            en = en.masked_fill(mask, -float("inf"))
        w = F.softmax(en, dim=1)
        ctx = torch.bmm(w.unsqueeze(1), mem).squeeze(1)
        cum = cum + w
        hd = torch.tanh(s.project_to_hidden[0].linear_layer(torch.cat([hid, ctx], -1)))
        logits.append(s.project_to_n_symbols(hd))
        aligns.append(w)
    return ctc, torch.stack(logits, 1), torch.stack(aligns, 1)


def main():
    from helpers import fill_module
    net = fill_module(ASRCNN(n_token=178, token_embedding_dim=512), "asr.").eval().cuda()
    out = {"T_mel": T_MEL, "L": T_MEL // 2, "T_text": T_TEXT, "reps": REPS, "cases": {}}
    for B in (2, 8):
        mel = torch.from_numpy(np.stack([synth.normal(f"ab:mel:{b}", (80, T_MEL)) for b in range(B)])).cuda()
        tok = torch.from_numpy(4 + (synth.hash_u01(f"ab:tok:{B}", B * T_TEXT) * 174).astype(np.int64)).view(B, -1).cuda()
        unk = torch.from_numpy(synth.hash_u01(f"ab:unk:{B}", B * T_TEXT) < 0.1).view(B, -1)
        mel_len = torch.tensor([T_MEL - 40 * b for b in range(B)])
        txt_len = torch.tensor([T_TEXT - 7 * b for b in range(B)])
        mask = (torch.arange(T_MEL // 2)[None, :] + 1 > (mel_len // 2)[:, None]).cuda()
        unk_dev = unk.cuda()
        with torch.no_grad():
            _, _, attn = net(mel, mask, tok, unk_mask=unk)
            ref = eager_forward(net, mel, mask, tok, unk_dev)
        a = attn[:, 1:].contiguous()
        search = lambda: maximum_path(a, mask_from_lens(a, txt_len, mel_len // 2))  # noqa: E731
        r = {"err_vs_eager": {k: float((x - y).abs().max()) for k, x, y in
                              zip(("ctc", "s2s_logit", "attn"), net(mel, mask, tok, unk_mask=unk), ref)}}
        with torch.no_grad():
            r["conv_stack"] = timed(lambda: net(mel))
            r["forward"] = timed(lambda: net(mel, mask, tok, unk_mask=unk))
            r["search"] = timed(search)
            r["total"] = timed(lambda: (net(mel, mask, tok, unk_mask=unk), search()))
            r["eager_forward"] = timed(lambda: eager_forward(net, mel, mask, tok, unk_dev))
        dec = r["forward"]["median_ms"] - r["conv_stack"]["median_ms"]
        r["decoder_ms"] = dec
        r["decoder_us_per_step"] = 1000.0 * dec / (T_TEXT + 1)
        out["cases"][f"B{B}"] = r
        print(f"B={B}: forward {r['forward']['median_ms']:.3f} ms (conv stack {r['conv_stack']['median_ms']:.3f}, decoder "
              f"{dec:.3f} = {r['decoder_us_per_step']:.1f} us/step), search {r['search']['median_ms']:.3f} ms, total "
              f"{r['total']['median_ms']:.3f} ms; eager torch forward {r['eager_forward']['median_ms']:.3f} ms; "
              f"max-abs vs eager {r['err_vs_eager']}")
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles")  # (an output directory may be given)
    os.makedirs(dst, exist_ok=True)
    with open(os.path.join(dst, "aligner_bench.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
