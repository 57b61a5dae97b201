"""Golden fixtures for the text aligner (Modules/ASR/models.py ASRCNN), made by running the REFERENCE code on the CPU:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_aligner.py

Imports /root/reference/Modules/ASR/models.py read-only; its layers.py imports torchaudio for create_dct alone (absent
here): stubbed with the formula (stts2_mi355x.asr.create_dct).  Every parameter comes from stts2_mi355x/synth.py
synth_param("asr." + key), the mels from synth.normal (zero beyond each utterance's length, as a padded batch), the
tokens from synth.hash_u01; the module runs in eval mode under no_grad.  The reference draws its unknown-token mask
with torch.rand inside forward: the seed set right before the call makes that draw the stored `unk_mask`.  Stores DATA
only (tests/golden/aligner_*.npz, aligner_keys.json), with each output's fp32-vs-fp64 difference from a .double()
copy of the module run with the same mask.
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
from stts2_mi355x.asr import create_dct  # noqa: E402

BIG, DEFAULT = (178, 512), (35, 256)  # (n_token, token_embedding_dim): the config's, the constructor's defaults
# (B, T_mel, T_text, mel lengths or None = no padding mask, text lengths, cfg)
CASES = (
    (1, 2, 1, (2,), (1,), BIG),
    (2, 14, 3, (14, 6), (3, 2), DEFAULT),
    (3, 41, 9, (41, 26, 33), (9, 6, 7), BIG),
    (2, 150, 40, None, (40, 31), BIG),
    (1, 300, 70, (300,), (70,), BIG),
)


def case_name(B, T, Tt):
    return f"aligner_B{B}_T{T}_Tt{Tt}.npz"


def stub(name, **attrs):
    m = types.ModuleType(name)
    m.__spec__ = importlib.machinery.ModuleSpec(name, None)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def inputs(B, T, Tt, mel_lens, n_token):
    mel = np.stack([synth.normal(f"aligner:mel:{b}:{T}", (80, T)) for b in range(B)])
    if mel_lens is not None:
        for b, n in enumerate(mel_lens):
            mel[b, :, n:] = 0.0
    tok = np.stack([4 + (synth.hash_u01(f"aligner:tok:{b}:{Tt}", Tt) * (n_token - 4)).astype(np.int64) for b in range(B)])
    return mel, tok


def make_module(n_token, emb):
    from Modules.ASR.models import ASRCNN
    torch.manual_seed(0)
    net = ASRCNN(input_dim=80, hidden_dim=256, n_token=n_token, n_layers=6, token_embedding_dim=emb).eval()
    sd = {}
    for k, v in net.state_dict().items():
        sd[k] = v if synth.is_fixed_buffer(k) else torch.from_numpy(synth.synth_param("asr." + k, tuple(v.shape)))
    net.load_state_dict(sd, strict=True)
    return net


def main():
    ta = stub("torchaudio")
    ta.functional = stub("torchaudio.functional", create_dct=lambda n_mfcc, n_mels, norm: create_dct(n_mfcc, n_mels))
    keys = {}
    for cfg in (BIG, DEFAULT):
        net = make_module(*cfg)
        keys["%d_%d" % cfg] = [[k, list(v.shape)] for k, v in net.state_dict().items()]
        assert len(keys["%d_%d" % cfg]) == 143
    with open(os.path.join(HERE, "aligner_keys.json"), "w") as f:
        json.dump(keys, f, indent=0)
    informative = False
    for i, (B, T, Tt, mel_lens, text_lens, cfg) in enumerate(CASES):
        net, net64 = make_module(*cfg), make_module(*cfg).double()
        mel, tok = inputs(B, T, Tt, mel_lens, cfg[0])
        L = (T + 1) // 2
        mask = None
        if mel_lens is not None:  # train.py:203: length_to_mask(mel_input_length // 2)
            mask = torch.arange(L)[None, :] + 1 > (torch.tensor(mel_lens) // 2)[:, None]
        x, t = torch.from_numpy(mel), torch.from_numpy(tok)
        seed = 100 + i
        torch.manual_seed(seed)
        unk = torch.rand(t.shape) < 0.1
        with torch.no_grad():
            torch.manual_seed(seed)
            ctc, s2s, attn = net(x, mask, t)
            torch.manual_seed(seed)
            ctc64, s2s64, attn64 = net64(x.double(), mask, t)
        rec = {"ctc": ctc.numpy(), "s2s_logit": s2s.numpy(), "attn": attn.numpy(), "unk_mask": unk.numpy(),
               "tokens": tok, "text_lens": np.asarray(text_lens, np.int64),
               "mel_lens": np.asarray(mel_lens if mel_lens is not None else (-1,), np.int64)}
        for k, a, b in (("ctc", ctc, ctc64), ("s2s_logit", s2s, s2s64), ("attn", attn, attn64)):
            rec[k + "_fp32_vs_fp64"] = np.float64((a.double() - b).abs().max().item())
        path = os.path.join(HERE, case_name(B, T, Tt))
        np.savez_compressed(path, **rec)
        wmax = attn.max(dim=2).values  # [B, Tt + 1]: the largest weight of every step
        valid = (~mask).sum(1).clamp(min=1).tolist() if mask is not None else [L] * B
        print(path, os.path.getsize(path), "unk", int(unk.sum()), "max weight per step (utterance 0):",
              np.round(wmax[0].numpy(), 3).tolist()[:12], "fp32 vs fp64",
              {k: v for k, v in rec.items() if k.endswith("fp64")})
        for b in range(B):
            if valid[b] > 2 and bool(((wmax[b] >= 2.0 / valid[b]) & (wmax[b] <= 0.999)).any()):
                informative = True
    if not informative:
        raise SystemExit("every step's largest attention weight is < 2 / L or > 0.999: rescale the asr.* synthesis rules")


if __name__ == "__main__":
    main()
