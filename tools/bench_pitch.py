"""The training step's two regression targets on the HIP path (train.py:260-262): JDCNet.forward + log_norm on the
cropped mel, at the train-step benches' crop (B = 2 segments of 93,000 samples = 310 mel frames at hop 300).
Per dtype: the median of --iters hipEvent times after --warmup calls, with max - min, then one profiled call for the
conv engine's per-launch split (stts_profile_*; the pooling, staging, BiLSTM and head launches are the remainder).

    python tools/bench_pitch.py [--segments 2] [--frames 310] [--iters 20] [--warmup 5] [--out profiles/pitch_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "styletts2-lite_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402


def conv_gflop(B, T):
    """Algorithmic conv + LSTM-projection work of one forward (2 flops per multiply-add)."""
    f, w = 0.0, 80
    f += 2.0 * B * T * w * 9 * (1 * 64 + 64 * 64)
    for cin, cout in ((64, 128), (128, 192), (192, 256)):
        w //= 2
        f += 2.0 * B * T * w * (9 * cin * cout + 9 * cout * cout + cin * cout)
    f += 2.0 * B * T * 2 * (512 * 1024 + 256 * 1024)
    return f / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=2)
    ap.add_argument("--frames", type=int, default=310)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from helpers import fill_module
    from stts2_mi355x import engine, prosody, synth
    from stts2_mi355x.jdc import JDCNet
    from stts2_mi355x.losses import log_norm
    torch.cuda.set_device(0)
    net = fill_module(JDCNet(num_class=1, seq_len=192), "jdc.").eval().cuda()
    B, T = a.segments, a.frames
    gt = torch.from_numpy(np.stack([synth.normal(f"pitch:mel:{b}:{T}", (80, T)) for b in range(B)])).cuda()
    line = {"workload": f"JDCNet.forward + log_norm, {B} segments x {T} mel frames", "alg_gflop": conv_gflop(B, T)}

    def call(dtype):
        f0, _, _ = net(gt.unsqueeze(1), dtype=dtype)
        return f0, log_norm(gt.unsqueeze(1)).squeeze(1)

    for dtype in ("fp32", "bf16x3"):
        for _ in range(a.warmup):
            call(dtype)
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call(dtype)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        engine.profile_enable(True)
        call(dtype)
        torch.cuda.synchronize()
        launches = engine.profile_launches()
        engine.profile_enable(False)
        conv_ms = sum(r["ms"] for r in launches)
        line[dtype] = {"ms": float(np.median(ts)), "spread_ms": float(max(ts) - min(ts)), "iters": a.iters,
                       "conv_engine_ms": conv_ms,
                       "conv_launches": [{k: r[k] for k in ("kernel", "rows", "N", "Cin", "taps", "ms")} for r in launches]}
    prosody.check_pending()
    print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(line, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
