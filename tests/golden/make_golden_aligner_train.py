"""Golden fixtures for training the whole text aligner (Modules/ASR/models.py ASRCNN), made by running the REFERENCE
code on the CPU in TRAIN mode with torch autograd, in fp32 and in fp64:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_aligner_train.py

(The reference's eval mode cannot be back-propagated: ConvBlock's `x += res` overwrites the ReLU's saved output when
Dropout is the identity.)  The reference is imported read-only as make_golden_aligner.py does (torchaudio stubbed).
Parameters are synth.synth_param("asr." + key) with n_token = 35 and embedding 256 (the constructor's defaults: the
files stay under the size limit); mels and tokens are make_golden_aligner.inputs' (synth.normal, zero past each
length).  torch.nn.functional.dropout is replaced for the run by injected masks in call order: calls 0-35, the
ConvBlocks' nn.Dropout(0.2), take synth.dropout_mask(k, shape, p) in the reference's [B, 256, L] layout; the S2S
decoder's F.dropout(hidden, 0.5) of step j takes [:, j] of synth.dropout_mask(36, (B, Tt + 1, 128), 0.5), the one call
over all steps of the HIP path (training.set_dropout_masks hands it the same masks).  The unknown-token mask is the
reference's own torch.rand draw under a fixed seed, stored as drawn.  Probe loss: sum(ctc P_c) + sum(s2s_logit P_l) +
sum(s2s_attn P_a) with synth.normal probes.

Stores DATA only (tests/golden/aligner_train_<case>.npz): the three outputs in fp32 with their fp32-vs-fp64
differences, and for all 142 parameters NS = 128 sampled gradient values from the fp64 run (the truth) and the fp32
run, in the f64. / f32. layout test_gpu_train_pred._check_fixture reads (128, not 256, keeps a file near 0.5 MB).
_check_fixture caps the module-normwise error at 1e-4; that bar is only fair if the reference's own fp32 run sits well
inside it, so this script asserts that every tensor of every case is within half of it (5e-5) and prints the worst.
"""
from __future__ import annotations

import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
warnings.filterwarnings("ignore")

import make_golden_aligner as mga  # noqa: E402  (also puts the package and the reference on sys.path)
from stts2_mi355x import synth  # noqa: E402
from stts2_mi355x.asr import create_dct  # noqa: E402

N_TOKEN, EMB, D = mga.DEFAULT[0], mga.DEFAULT[1], 128
NS = 128
NORM_CAP = 5e-5  # half of _check_fixture's module-normwise cap
# name, B, T_mel, Tt, mel lengths (None: full, no padding mask), text lengths
CASES = (
    ("A", 1, 2, 1, None, (1,)),                    # L = 1: one frame per group; every dilated tap in padding
    ("B", 2, 14, 3, (14, 6), (3, 2)),              # L = 7 < dilation 9; masked memory
    # The mel lengths of C and D are chosen for the stack's 37 ReLUs.  One ReLU decision taken differently from the
    # fp64 run moves a weight gradient by 2e-3 to 1e-2 of the module's largest (the decision's derivative is a step),
    # 20 to 100 times the bar the fixtures are read under, and any fp32 forward takes it differently when the
    # pre-activation is within its rounding error of zero (about 1e-6 after 36 convs).  With (41, 26, 33) the smallest
    # fp64 |pre-activation| of C's 0.6 M is 6.4e-7; with both mels full the reference's own fp32 run flips one of D's
    # 2.8 M (5.6e-7) and misses the 5e-5 condition below by a factor of 100.  Utterances do not see each other
    # (GroupNorm is per sample), so each length was picked on its own, from a scan of the fp64 run over 22 (C) and
    # 60 (D) lengths, as the one whose smallest |pre-activation| is largest; `min_preact` records it per case.
    ("C", 3, 41, 9, (39, 27, 40), (9, 6, 7)),      # odd T, L = ceil(T / 2) = 21; smallest |pre-activation| 1.2e-5
    ("D", 2, 300, 5, (132, 276), (5, 5)),          # L = 150: several GroupNorm row slices and conv tiles; 4.0e-6
)
_MIN_PREACT = []


def probes(B, L, Tt):
    return (synth.normal(f"altrain:probe:c:{B}:{L}:{Tt}", (B, L, N_TOKEN)),
            synth.normal(f"altrain:probe:l:{B}:{L}:{Tt}", (B, Tt + 1, N_TOKEN)),
            synth.normal(f"altrain:probe:a:{B}:{L}:{Tt}", (B, Tt + 1, L)))


def probe_idx(key, size):
    return np.minimum((synth.hash_u01("altrain:idx:" + key, NS) * size).astype(np.int64), size - 1)


class _InjectedDropout:
    """torch.nn.functional.dropout replaced by the injected masks, in call order (see the module docstring)."""

    def __init__(self, B, steps):
        self.k, self.s2s = 0, synth.dropout_mask(36, (B, steps, D), 0.5)

    def __call__(self, x, p=0.5, training=True, inplace=False):
        if not training or p == 0:
            return x
        if self.k < 36:
            m = synth.dropout_mask(self.k, tuple(x.shape), p)
        else:
            m = self.s2s[:, self.k - 36]
        self.k += 1
        return x * torch.from_numpy(m).to(x.dtype) / (1 - p)


def _relu(self, x):
    """nn.ReLU.forward, recording the smallest |pre-activation| (see CASES)."""
    _MIN_PREACT.append(float(x.detach().abs().min()))
    return torch.relu(x)


def run(dt, B, T, Tt, mel_lens, seed):
    import torch.nn.functional as F
    net = mga.make_module(N_TOKEN, EMB).to(dt).train()
    mel, tok = mga.inputs(B, T, Tt, mel_lens, N_TOKEN)
    L = (T + 1) // 2
    mask = None
    if mel_lens is not None:  # train.py:203: length_to_mask(mel_input_length // 2)
        mask = torch.arange(L)[None, :] + 1 > (torch.tensor(mel_lens) // 2)[:, None]
    saved, saved_relu = F.dropout, torch.nn.ReLU.forward
    F.dropout = _InjectedDropout(B, Tt + 1)
    torch.nn.ReLU.forward = _relu
    del _MIN_PREACT[:]
    try:
        torch.manual_seed(seed)
        ctc, s2s, attn = net(torch.from_numpy(mel).to(dt), mask, torch.from_numpy(tok))
        ncalls = F.dropout.k
    finally:
        F.dropout, torch.nn.ReLU.forward = saved, saved_relu
    assert ncalls == 36 + Tt + 1 and len(_MIN_PREACT) == 37, (ncalls, len(_MIN_PREACT))
    pc, pl, pa = (torch.from_numpy(p).to(dt) for p in probes(B, L, Tt))
    ((ctc * pc).sum() + (s2s * pl).sum() + (attn * pa).sum()).backward()
    grads = {k: p.grad for k, p in net.named_parameters()}
    assert len(grads) == 142 and all(g is not None for g in grads.values())
    return (ctc.detach(), s2s.detach(), attn.detach()), grads, mask, tok


def main():
    ta = mga.stub("torchaudio")
    ta.functional = mga.stub("torchaudio.functional", create_dct=lambda n_mfcc, n_mels, norm: create_dct(n_mfcc, n_mels))
    worst = (0.0, "")
    for i, (name, B, T, Tt, mel_lens, text_lens) in enumerate(CASES):
        seed = 400 + i
        torch.manual_seed(seed)
        unk = torch.rand(B, Tt) < 0.1
        out32, g32, mask, tok = run(torch.float32, B, T, Tt, mel_lens, seed)
        out64, g64, _, _ = run(torch.float64, B, T, Tt, mel_lens, seed)
        min_preact = min(_MIN_PREACT)  # (of the fp64 run)
        names = list(g64)
        rec = {"names": np.array(names), "B": np.int64(B), "T": np.int64(T), "L": np.int64((T + 1) // 2),
               "Tt": np.int64(Tt), "unk_mask": unk.numpy(), "tokens": tok, "min_preact": np.float64(min_preact),
               "mel_lens": np.asarray(mel_lens if mel_lens is not None else (-1,), np.int64),
               "text_lens": np.asarray(text_lens, np.int64)}
        for k, a, b in zip(("ctc", "s2s_logit", "attn"), out32, out64):
            rec[k] = a.numpy()
            rec[k + "_fp32_vs_fp64"] = np.float64((a.double() - b).abs().max().item())
        idx = [probe_idx(k, g64[k].numel()) for k in names]
        rec["f64.idx"] = np.stack(idx)
        rec["f64.maxabs"] = np.array([g64[k].abs().max().item() for k in names])
        rec["f64.val"] = np.stack([g64[k].reshape(-1).numpy()[ix] for k, ix in zip(names, idx)])
        rec["f32.val"] = np.stack([g32[k].reshape(-1).double().numpy()[ix] for k, ix in zip(names, idx)])
        if mask is not None:
            assert float(out64[2][mask[:, None, :].expand_as(out64[2])].abs().max()) == 0.0
        gm = rec["f64.maxabs"].max()
        case_worst = (0.0, "")
        for j, k in enumerate(names):
            en = np.abs(rec["f32.val"][j] - rec["f64.val"][j]).max() / gm
            case_worst = max(case_worst, (float(en), k))
        assert case_worst[0] <= NORM_CAP, (name, case_worst)  # (not within it: change the case's seed or lengths)
        worst = max(worst, (case_worst[0], f"{name} {case_worst[1]}"))
        path = os.path.join(HERE, f"aligner_train_{name}.npz")
        np.savez_compressed(path, **rec)
        assert os.path.getsize(path) < 1 << 20, os.path.getsize(path)
        print(path, os.path.getsize(path), "unk", int(unk.sum()), f"smallest |pre-activation| {min_preact:.2e}",
              "fp32 reference module-normwise worst",
              f"{case_worst[0]:.2e} ({case_worst[1]})", "outputs fp32 vs fp64",
              {k: float(v) for k, v in rec.items() if k.endswith("fp64")})
    print(f"worst fp32 reference module-normwise error over all cases: {worst[0]:.2e} ({worst[1]}); cap {NORM_CAP:.0e}")


if __name__ == "__main__":
    main()
