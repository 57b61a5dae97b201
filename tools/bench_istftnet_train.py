"""One fine-tune step with the iSTFTNet decoder (n_fft 20, hop 5, rates [10, 6]) on one MI355X at the config-5 shape:
B = 2 segments of 155 asr frames = 93,000 samples, TrainStep (decoder forward, D step, G step, AdamW), eager.

    python tools/bench_istftnet_train.py [--steps 20] [--warmup 5] [--dtypes bf16,bf16x3,fp32]
                                         [--out profiles/istftnet_train_bench.json]

Prints one JSON line per dtype (median, min and max of hipEvent-timed steps, wall and host issue time) and, with
--out, writes the list to that file.  Inputs are synthetic and resident in HBM, formula weights.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "styletts2-lite_amd"), os.path.join(ROOT, "tests")]
import torch  # noqa: E402


def run(dtype, B, T, steps, warmup):
    from helpers import fill_module, make_decoder
    from stts2_mi355x import synth
    from stts2_mi355x.discriminators import MultiPeriodDiscriminator, MultiResSpecDiscriminator
    from stts2_mi355x.trainstep import TrainStep
    dec, cfg = make_decoder("istftnet")
    dec = dec.cuda().eval()
    mpd = fill_module(MultiPeriodDiscriminator(), "mpd.").cuda().train()
    msd = fill_module(MultiResSpecDiscriminator(), "msd.").cuda().train()
    ins = [torch.from_numpy(a).cuda().requires_grad_(True) for a in synth.decoder_inputs(B, T, tag="train")]
    L = 2 * T * dec.generator.upsample_scale
    wav = torch.from_numpy(synth.waves(B, L, 7)).cuda()
    step = TrainStep(dec, mpd, msd, dtype=dtype)
    for i in range(max(warmup, 1)):
        step(*ins, wav, seed=100 + i)
    torch.cuda.synchronize()
    ev, host = [], []
    t0 = time.perf_counter()
    for i in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        h0 = time.perf_counter()
        out = step(*ins, wav, seed=1000 + i)
        host.append((time.perf_counter() - h0) * 1e3)
        b.record()
        ev.append((a, b))
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / steps * 1e3
    ms = [x.elapsed_time(y) for x, y in ev]
    return {"metric": "istftnet train step (eager)", "dtype": dtype, "B": B, "T_frames": T,
            "n_fft": cfg["gen_istft_n_fft"], "hop": cfg["gen_istft_hop_size"], "samples_per_utt": L,
            "ms_per_step_median": round(statistics.median(ms), 2), "ms_per_step_min": round(min(ms), 2),
            "ms_per_step_max": round(max(ms), 2), "ms_max_minus_min": round(max(ms) - min(ms), 2),
            "ms_per_step_wall": round(wall, 2), "host_ms_per_step": round(statistics.median(host), 2), "steps": steps,
            "warmup": warmup, "losses": {k: float(out[k]) for k in ("d_loss", "loss_mel", "loss_gen_all")},
            "max_mem_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dtypes", default="bf16,bf16x3,fp32")
    ap.add_argument("--B", type=int, default=2)
    ap.add_argument("--T", type=int, default=155)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for dt in a.dtypes.split(","):
        rows.append(run(dt, a.B, a.T, a.steps, a.warmup))
        print(json.dumps(rows[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
