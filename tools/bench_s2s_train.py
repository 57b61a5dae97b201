"""S2S decoder training timing at B = 2, L = 400, T_text = 150, fp32: the HIP training forward (stts_s2s_fwd_train),
its backward (stts_s2s_bwd), the forward that keeps no state (the plain decoder kernel: the difference is the cost
of saving), and forward + backward of the torch restatement (tests/s2s_ref.py) in fp32 through torch-ROCm ops on the
same device.  Also the per-tensor gradient errors of both against the restatement in fp64.

    python tools/bench_s2s_train.py [out_dir]   -> profiles/s2s_train_bench.json, profiles/s2s_train_dtype_err.txt

Warm-up, then the median of 20 timed calls with max - min, hipEvents on the launch stream."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "styletts2-lite_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from stts2_mi355x import synth  # noqa: E402
from stts2_mi355x.asr import ASRCNN  # noqa: E402

B, L, T_TEXT, D, REPS, WARM = 2, 400, 150, 128, 20, 3


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


def main():
    from helpers import fill_module
    from s2s_ref import KEYS, s2s_forward
    net = fill_module(ASRCNN(n_token=178, token_embedding_dim=512), "asr.").asr_s2s.eval().cuda()
    mem = torch.from_numpy(synth.normal("sb:mem", (B, L, D))).cuda()
    tok = torch.from_numpy(4 + (synth.hash_u01("sb:tok", B * T_TEXT) * 174).astype(np.int64)).view(B, -1).cuda()
    unk = torch.from_numpy(synth.hash_u01("sb:unk", B * T_TEXT) < 0.1).view(B, -1)
    mask = (torch.arange(L)[None, :] >= torch.tensor([L, L - 20])[:, None]).cuda()
    probes = [torch.from_numpy(synth.normal(f"sb:probe:{k}", shp)).cuda() for k, shp in
              (("h", (B, T_TEXT + 1, D)), ("l", (B, T_TEXT + 1, 178)), ("a", (B, T_TEXT + 1, L)))]
    unk_dev = unk.cuda()

    def hip(m):
        return net(m, mask, tok, unk_mask=unk)

    def ref(dt, m, ps):
        return s2s_forward(ps, m, mask, tok, unk_dev)

    def grads_of(out, m, ps):
        return torch.autograd.grad(sum((o * p.to(o.dtype)).sum() for o, p in zip(out, probes)), [m, *ps])

    ps32 = [p.detach().requires_grad_(True) for _, p in net.named_parameters()]
    m32 = mem.clone().requires_grad_(True)
    out = {"B": B, "L": L, "T_text": T_TEXT, "reps": REPS}
    with torch.no_grad():
        out["hip_forward_no_state"] = timed(lambda: hip(mem))
    out["hip_forward_train"] = timed(lambda: hip(m32))
    o = hip(m32)
    loss = sum((a * p).sum() for a, p in zip(o, probes))
    out["hip_backward"] = timed(lambda: torch.autograd.grad(loss, [m32, *net.parameters()], retain_graph=True))
    out["hip_forward_backward"] = timed(lambda: grads_of(hip(m32), m32, list(net.parameters())))
    out["torch_forward"] = timed(lambda: ref(torch.float32, m32, ps32))
    out["torch_forward_backward"] = timed(lambda: grads_of(ref(torch.float32, m32, ps32), m32, ps32))
    out["save_overhead_ms"] = out["hip_forward_train"]["median_ms"] - out["hip_forward_no_state"]["median_ms"]
    out["speedup_forward_backward"] = (out["torch_forward_backward"]["median_ms"]
                                       / out["hip_forward_backward"]["median_ms"])
    ps64 = [p.detach().double().requires_grad_(True) for p in ps32]
    m64 = mem.double().requires_grad_(True)
    g64 = grads_of(ref(torch.float64, m64, ps64), m64, ps64)
    g32 = grads_of(ref(torch.float32, m32, ps32), m32, ps32)
    gh = grads_of(hip(m32), m32, list(net.parameters()))
    lines = ["tensor  max|g64|  HIP fp32 vs fp64 (rel. to the tensor's max)  torch fp32 vs fp64"]
    for k, a, b, c in zip(("dmemory",) + KEYS, g64, gh, g32):
        s = float(a.abs().max())
        lines.append(f"{k}  {s:.3e}  {float((b.double() - a).abs().max()) / s:.2e}  "
                     f"{float((c.double() - a).abs().max()) / s:.2e}")
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles")  # (an output directory may be given)
    os.makedirs(dst, exist_ok=True)
    with open(os.path.join(dst, "s2s_train_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
    with open(os.path.join(dst, "s2s_train_dtype_err.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps(out))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
