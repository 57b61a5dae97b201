"""Gradient fixtures for the trainable iSTFTNet decoder, made by running the REFERENCE module's own
autograd in the survey container (never on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_istftnet_train.py

Imports /root/reference/Modules/istftnet.py read-only, builds the `Decoder` as make_golden.py does
(ISTFT_CFG: n_fft 20, hop 5, rates [10, 6]; formula weights of stts2_mi355x/synth.py by state-dict key), in
eval mode and in float64, runs forward(asr, F0_curve, N, s) with grad on the formula inputs and with the
reference's randn_like / rand draws replaced by the formula noise (make_golden.NoisePatch), and
backpropagates loss = (out * R).sum() with R = randn(out.shape, float64) from
torch.Generator().manual_seed(seed).

The sine generator keeps the reference's own float32: `generator.m_source.l_sin_gen.forward` is called
with its input cast to float32 and its outputs cast back (it runs under no_grad, istftnet.py:483-484, so
this changes no graph).  A checkpoint is float32, so the phase accumulation of SineGen is float32 in every
real run; the oracle (oracle.sine_source) does the same in its float64 runs.

Stored per case as .npz DATA (tests/golden/istftnet_train_*.npz): the loss, R's seed, the four input
gradients in full, for every parameter with a gradient its sum, L2 norm, max-abs and the values at 64
fixed-stride indices, and the names of the parameters whose gradient is None (the reference computes the
harmonic source and its STFT under no_grad, :544-550: generator.m_source.l_linear).  The case list goes to
tests/golden/meta_istftnet_train.json.
"""
from __future__ import annotations

import json
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import ISTFT_CFG, REF, NoisePatch, fill, synth  # noqa: E402

sys.path.insert(0, REF)
warnings.filterwarnings("ignore")

CASES = ((4, 2), (7, 1))  # (T, B)
N_SAMPLES = 64
R_SEED = 20250


def sample_idx(numel: int) -> np.ndarray:
    """64 fixed-stride flat indices of a tensor of `numel` values (wrapping for tensors below 64 values)."""
    if numel >= N_SAMPLES:
        return np.arange(N_SAMPLES, dtype=np.int64) * (numel // N_SAMPLES)
    return np.arange(N_SAMPLES, dtype=np.int64) % numel


def run(T, B):
    from Modules.istftnet import Decoder
    torch.manual_seed(0)
    dec = fill(Decoder(dim_in=512, style_dim=128, dim_out=80, **ISTFT_CFG)).eval().double()
    sg = dec.generator.m_source.l_sin_gen
    sg_forward = sg.forward
    sg.forward = lambda f0: tuple(o.double() for o in sg_forward(f0.float()))
    ins = [torch.from_numpy(a).double().requires_grad_(True) for a in synth.decoder_inputs(B, T)]
    scale = int(np.prod(ISTFT_CFG["upsample_rates"])) * ISTFT_CFG["gen_istft_hop_size"]
    with NoisePatch(synth.source_noise(B, 2 * T * scale)):
        out = dec(*ins)
    R = torch.randn(out.shape, generator=torch.Generator().manual_seed(R_SEED), dtype=torch.float64)
    loss = (out * R).sum()
    loss.backward()
    res = {"loss": np.float64(loss.item()), "r_seed": np.int64(R_SEED), "B": np.int64(B), "T": np.int64(T),
           "out_shape": np.asarray(out.shape, np.int64)}
    for k, t in zip(("asr", "F0_curve", "N", "s"), ins):
        res["grad_in." + k] = t.grad.numpy()
    names, none, sums, l2s, mx, vals = [], [], [], [], [], []
    for k, p in dec.named_parameters():
        if p.grad is None:
            none.append(k)
            continue
        g = p.grad.detach().reshape(-1)
        names.append(k)
        sums.append(float(g.sum()))
        l2s.append(float(g.norm()))
        mx.append(float(g.abs().max()))
        vals.append(g[torch.from_numpy(sample_idx(g.numel()))].numpy())
    res.update({"names": np.asarray(names), "none": np.asarray(none), "sum": np.asarray(sums), "l2": np.asarray(l2s),
                "maxabs": np.asarray(mx), "val": np.stack(vals)})
    return res


def main():
    torch.set_num_threads(8)
    meta = {"generator": "tests/golden/make_golden_istftnet_train.py", "n_samples": N_SAMPLES, "cases": {}}
    for T, B in CASES:
        r = run(T, B)
        name = f"istftnet_train_T{T}_B{B}"
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **r)
        meta["cases"][name] = {"n_fft": ISTFT_CFG["gen_istft_n_fft"], "hop": ISTFT_CFG["gen_istft_hop_size"], "T": T,
                               "B": B, "r_seed": R_SEED, "loss": float(r["loss"]), "n_params": int(len(r["names"])),
                               "no_grad": [str(k) for k in r["none"]], "grad_maxabs": float(r["maxabs"].max())}
        print(name, meta["cases"][name], flush=True)
    with open(os.path.join(HERE, "meta_istftnet_train.json"), "w") as f:
        json.dump(meta, f, indent=1)


if __name__ == "__main__":
    main()
