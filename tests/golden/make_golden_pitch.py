"""Golden fixtures for the pitch extractor (Modules/JDC/model.py JDCNet) and log_norm (utils.py:48-53), the two
regression targets of the fine-tune step (train.py:260-262), made by running the REFERENCE code on the CPU:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_pitch.py

Imports /root/reference/Modules/JDC/model.py (torch only) and utils.log_norm read-only; utils.py imports
monotonic_align, torchaudio, librosa and munch at module level (absent here, unused by log_norm): stubbed.  Every
parameter and BatchNorm statistic comes from stts2_mi355x/synth.py synth_param("jdc." + key), the mels from
synth.normal; the module runs in eval mode under no_grad.  Stores DATA only (tests/golden/pitch_*.npz,
pitch_keys.json).
"""
from __future__ import annotations

import importlib.machinery
import json
import os
import sys
import types
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

CASES = ((3, 1, 1), (1, 7, 1), (2, 12, 1), (2, 9, 5), (3, 130, 1))  # (B, T, num_class)


def stub(name, **attrs):
    if name in sys.modules:
        return sys.modules[name]
    m = types.ModuleType(name)
    m.__spec__ = importlib.machinery.ModuleSpec(name, None)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def import_log_norm():
    ma = stub("monotonic_align", maximum_path=None, mask_from_lens=None)
    ma.core = stub("monotonic_align.core", maximum_path_c=None)
    ta = stub("torchaudio")
    ta.transforms = types.SimpleNamespace(MelSpectrogram=None, Resample=None)
    stub("librosa")

    class Munch(dict):
        __getattr__ = dict.get
    stub("munch", Munch=Munch)
    import utils  # noqa
    return utils.log_norm


def mels(B, T):
    return np.stack([synth.normal(f"pitch:mel:{b}:{T}", (80, T)) for b in range(B)])


def make_module(num_class):
    from Modules.JDC.model import JDCNet
    torch.manual_seed(0)
    net = JDCNet(num_class=num_class, seq_len=192).eval()
    sd = {}
    for k, v in net.state_dict().items():
        if synth.is_fixed_buffer(k):
            sd[k] = v
        else:
            sd[k] = torch.from_numpy(synth.synth_param("jdc." + k, tuple(v.shape)))
    net.load_state_dict(sd, strict=True)
    return net


def forward64(net, x):
    """JDCNet.forward (model.py:111-137) on a .double() module: the same calls without forward's x.float()."""
    seq_len = x.shape[-1]
    h = net.res_block3(net.res_block2(net.res_block1(net.conv_block(x.transpose(-1, -2)))))
    h = net.pool_block[2](net.pool_block[1](net.pool_block[0](h)))
    h = h.permute(0, 2, 1, 3).contiguous().view((-1, seq_len, 512))
    h, _ = net.bilstm_classifier(h)
    h = net.classifier(h.contiguous().view((-1, 512))).view((-1, seq_len, net.num_class))
    return torch.abs(h.squeeze())


def main():
    log_norm = import_log_norm()
    net1 = make_module(1)
    keys = [[k, list(v.shape)] for k, v in net1.state_dict().items()]
    assert len(keys) == 77
    with open(os.path.join(HERE, "pitch_keys.json"), "w") as f:
        json.dump(keys, f, indent=0)
    for B, T, nc in CASES:
        net = net1 if nc == 1 else make_module(nc)
        mel = mels(B, T)
        x = torch.from_numpy(mel)
        with torch.no_grad():
            f0, gan, pool = net(x.unsqueeze(1))
            n_real = log_norm(x.unsqueeze(1)).squeeze(1)
            net64 = make_module(nc).double()
            f064 = forward64(net64, x.double().unsqueeze(1))
        rec = {"f0": f0.numpy(), "pool_out": pool.numpy(), "n_real": n_real.numpy(),
               "f0_fp32_vs_fp64": np.float64((f0.double() - f064).abs().max().item())}
        if T <= 12:
            rec["gan_feature"] = gan.numpy()
        path = os.path.join(HERE, f"pitch_B{B}_T{T}_C{nc}.npz")
        np.savez_compressed(path, **rec)
        print(path, os.path.getsize(path), {k: getattr(v, "shape", v) for k, v in rec.items()},
              "max|f0|", float(f0.abs().max()), "fp32 vs fp64", rec["f0_fp32_vs_fp64"])


if __name__ == "__main__":
    main()
