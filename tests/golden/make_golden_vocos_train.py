"""Gradient fixtures for the trainable Vocos decoder, made by running the REFERENCE module's own
autograd in the survey container (never on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_vocos_train.py

Imports /root/reference/Modules/vocos.py read-only, builds the `Decoder` as make_golden_vocos.py
does (formula weights of stts2_mi355x/synth.py by state-dict key), in eval mode and in float64, runs
forward(asr, F0_curve, N, s) with grad on the formula inputs and backpropagates
loss = (out * R).sum() with R = randn(out.shape, float64) from torch.Generator().manual_seed(seed).

Stored per case as .npz DATA (tests/golden/vocos_train_*.npz): the loss, R's seed, the four input
gradients in full, and for every parameter its gradient's sum, L2 norm, max-abs and the values at 64
fixed-stride indices (the full parameter gradients are ~30 M values).  The case list goes to
tests/golden/meta_vocos_train.json.
"""
from __future__ import annotations

import json
import os
import sys
import warnings

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "styletts2-lite_amd"))
sys.path.insert(0, REF)
warnings.filterwarnings("ignore")

from stts2_mi355x import synth  # noqa: E402

CASES = (  # (n_fft, hop, T, B)
    (1200, 300, 4, 2),
    (1024, 256, 7, 1),
)
N_SAMPLES = 64
R_SEED = 20240


def sample_idx(numel: int) -> np.ndarray:
    """64 fixed-stride flat indices of a tensor of `numel` values (wrapping for tensors below 64 values)."""
    if numel >= N_SAMPLES:
        return np.arange(N_SAMPLES, dtype=np.int64) * (numel // N_SAMPLES)
    return np.arange(N_SAMPLES, dtype=np.int64) % numel


def fill(module):
    sd = module.state_dict()
    new = {}
    for k, v in sd.items():
        new[k] = v if synth.is_fixed_buffer(k) else torch.from_numpy(synth.synth_param(k, tuple(v.shape)))
    module.load_state_dict(new, strict=True)
    return module


def run(n_fft, hop, T, B):
    from Modules.vocos import Decoder
    torch.manual_seed(0)
    dec = Decoder(dim_in=512, style_dim=128, dim_out=80, intermediate_dim=1536, num_layers=8,
                  gen_istft_n_fft=n_fft, gen_istft_hop_size=hop)
    dec = fill(dec).eval().double()
    ins = [torch.from_numpy(a).double().requires_grad_(True) for a in synth.decoder_inputs(B, T, tag="vocos")]
    out = dec(*ins)
    R = torch.randn(out.shape, generator=torch.Generator().manual_seed(R_SEED), dtype=torch.float64)
    loss = (out * R).sum()
    loss.backward()
    res = {"loss": np.float64(loss.item()), "r_seed": np.int64(R_SEED), "B": np.int64(B), "T": np.int64(T),
           "out_shape": np.asarray(out.shape, np.int64)}
    for k, t in zip(("asr", "F0_curve", "N", "s"), ins):
        res["grad_in." + k] = t.grad.numpy()
    names, sums, l2s, mx, vals = [], [], [], [], []
    for k, p in dec.named_parameters():
        g = p.grad.detach().reshape(-1)
        names.append(k)
        sums.append(float(g.sum()))
        l2s.append(float(g.norm()))
        mx.append(float(g.abs().max()))
        vals.append(g[torch.from_numpy(sample_idx(g.numel()))].numpy())
    res.update({"names": np.asarray(names), "sum": np.asarray(sums), "l2": np.asarray(l2s), "maxabs": np.asarray(mx),
                "val": np.stack(vals)})
    return res


def main():
    torch.set_num_threads(8)
    meta = {"generator": "tests/golden/make_golden_vocos_train.py", "n_samples": N_SAMPLES, "cases": {}}
    for n_fft, hop, T, B in CASES:
        r = run(n_fft, hop, T, B)
        name = f"vocos_train_n{n_fft}_T{T}_B{B}"
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **r)
        meta["cases"][name] = {"n_fft": n_fft, "hop": hop, "T": T, "B": B, "r_seed": R_SEED,
                               "loss": float(r["loss"]), "n_params": int(len(r["names"])),
                               "grad_maxabs": float(r["maxabs"].max())}
        print(name, meta["cases"][name], flush=True)
    with open(os.path.join(HERE, "meta_vocos_train.json"), "w") as f:
        json.dump(meta, f, indent=1)


if __name__ == "__main__":
    main()
