"""Golden fixtures for training the aligner's S2S decoder (Modules/ASR/models.py ASRS2S), made by running the
REFERENCE code on the CPU with torch autograd:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_s2s_train.py

Imports /root/reference/Modules/ASR/models.py read-only (torchaudio stubbed as make_golden_aligner.py does).  The
parameters are synth.synth_param("asr.asr_s2s." + key), what fill_module(net, "asr.") gives the drop-in's asr_s2s;
memory comes from synth.normal, the tokens from synth.hash_u01; the unknown-token mask is the reference's own
torch.rand draw under a fixed seed, stored as drawn.  In train mode the reference's F.dropout(hidden, 0.5) of step k
takes [:, k] of synth.dropout_mask(0, (B, Tt + 1, 128), 0.5), the mask training.set_dropout_masks hands the HIP path
for its one call over all steps.  Probe loss: sum(hidden P_h) + sum(logit P_l) + sum(attn P_a) with synth.normal
probes.  Stores DATA only (tests/golden/s2s_train_*.npz): the three outputs in fp32 with their fp32-vs-fp64
differences, and 256 sampled values of dmemory and of the 14 parameter gradients from the fp64 run (the truth) and
the fp32 run, in the f64. / f32. layout test_gpu_train_pred._check_fixture reads.
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

N_TOKEN, EMB, D = 35, 256, 128  # ASRCNN's constructor defaults: the 178 x 512 table alone would pass the file limit
NS = 256
# name, B, L, Tt, valid memory lengths (None: unmasked), text lengths, train mode
CASES = (
    ("A", 1, 1, 1, None, (1,), False),
    ("B", 2, 7, 3, (7, 3), (3, 2), False),
    ("Bdrop", 2, 7, 3, (7, 3), (3, 2), True),
    ("C", 3, 21, 9, (21, 13, 16), (9, 6, 7), False),
    ("D", 2, 150, 5, None, (5, 4), False),
)


def inputs(B, L, Tt, mem_lens):
    mem = np.stack([synth.normal(f"s2s:mem:{b}:{L}", (L, D)) for b in range(B)])
    tok = np.stack([4 + (synth.hash_u01(f"s2s:tok:{b}:{Tt}", Tt) * (N_TOKEN - 4)).astype(np.int64) for b in range(B)])
    mask = None
    if mem_lens is not None:
        mask = np.arange(L)[None, :] >= np.asarray(mem_lens)[:, None]
    return mem, tok, mask


def probes(B, L, Tt):
    return (synth.normal(f"s2s:probe:h:{B}:{L}:{Tt}", (B, Tt + 1, D)),
            synth.normal(f"s2s:probe:l:{B}:{L}:{Tt}", (B, Tt + 1, N_TOKEN)),
            synth.normal(f"s2s:probe:a:{B}:{L}:{Tt}", (B, Tt + 1, L)))


def probe_idx(key, size):
    return np.minimum((synth.hash_u01("s2s:idx:" + key, NS) * size).astype(np.int64), size - 1)


def make_module(dt):
    from Modules.ASR.models import ASRS2S
    torch.manual_seed(0)
    net = ASRS2S(embedding_dim=EMB, hidden_dim=D, n_token=N_TOKEN)
    sd = {k: torch.from_numpy(synth.synth_param("asr.asr_s2s." + k, tuple(v.shape))) for k, v in net.state_dict().items()}
    net.load_state_dict(sd, strict=True)
    return net.to(dt)


class _StepDropout:
    """F.dropout of decode step k: column k of the one mask over all steps."""

    def __init__(self, B, steps):
        self.mask, self.k = synth.dropout_mask(0, (B, steps, D), 0.5), 0

    def __call__(self, x, p=0.5, training=True, inplace=False):
        if not training or p == 0:
            return x
        m = torch.from_numpy(self.mask[:, self.k]).to(x.dtype)
        self.k += 1
        return x * m / (1 - p)


def run(dt, B, L, Tt, mem_lens, train, seed):
    import torch.nn.functional as F
    net = make_module(dt).train(train)
    mem, tok, mask = inputs(B, L, Tt, mem_lens)
    m = torch.from_numpy(mem).to(dt).requires_grad_(True)
    mk = None if mask is None else torch.from_numpy(mask)
    saved = F.dropout
    F.dropout = _StepDropout(B, Tt + 1)
    try:
        torch.manual_seed(seed)
        hidden, logit, attn = net(m, mk, torch.from_numpy(tok))
    finally:
        F.dropout = saved
    ph, pl, pa = (torch.from_numpy(p).to(dt) for p in probes(B, L, Tt))
    ((hidden * ph).sum() + (logit * pl).sum() + (attn * pa).sum()).backward()
    grads = {k: p.grad for k, p in net.named_parameters()}
    assert len(grads) == 14 and all(g is not None for g in grads.values())
    grads["dmemory"] = m.grad
    return (hidden.detach(), logit.detach(), attn.detach()), grads, mask


def main():
    ta = mga.stub("torchaudio")
    ta.functional = mga.stub("torchaudio.functional", create_dct=lambda n_mfcc, n_mels, norm: create_dct(n_mfcc, n_mels))
    informative = False
    for i, (name, B, L, Tt, mem_lens, text_lens, train) in enumerate(CASES):
        seed = 300 + i
        torch.manual_seed(seed)
        unk = torch.rand(B, Tt) < 0.1
        out32, g32, mask = run(torch.float32, B, L, Tt, mem_lens, train, seed)
        out64, g64, _ = run(torch.float64, B, L, Tt, mem_lens, train, seed)
        names = list(g64)
        rec = {"names": np.array(names), "B": np.int64(B), "L": np.int64(L), "Tt": np.int64(Tt),
               "train": np.bool_(train), "unk_mask": unk.numpy(), "tokens": inputs(B, L, Tt, mem_lens)[1],
               "mem_lens": np.asarray(mem_lens if mem_lens is not None else (-1,), np.int64),
               "text_lens": np.asarray(text_lens, np.int64)}
        for k, a, b in zip(("hidden", "logit", "attn"), out32, out64):
            rec[k] = a.numpy()
            rec[k + "_fp32_vs_fp64"] = np.float64((a.double() - b).abs().max().item())
        idx = [probe_idx(k, g64[k].numel()) for k in names]
        rec["f64.idx"] = np.stack(idx)
        rec["f64.maxabs"] = np.array([g64[k].abs().max().item() for k in names])
        rec["f64.val"] = np.stack([g64[k].reshape(-1).numpy()[ix] for k, ix in zip(names, idx)])
        rec["f32.val"] = np.stack([g32[k].reshape(-1).double().numpy()[ix] for k, ix in zip(names, idx)])
        if mask is not None:
            assert float(g64["dmemory"][torch.from_numpy(mask)].abs().max()) == 0.0
            assert float(out64[2][torch.from_numpy(mask)[:, None, :].expand_as(out64[2])].abs().max()) == 0.0
        # the fp32 reference itself inside the bars the tests hold the HIP path to
        gm = rec["f64.maxabs"].max()
        for j, k in enumerate(names):
            scale = max(rec["f64.maxabs"][j], 1e-3 * gm)
            er = np.abs(rec["f32.val"][j] - rec["f64.val"][j]).max() / scale
            assert er <= 1e-3, (name, k, er)
        path = os.path.join(HERE, f"s2s_train_{name}.npz")
        np.savez_compressed(path, **rec)
        assert os.path.getsize(path) < 200_000, os.path.getsize(path)
        wmax = out32[2].max(dim=2).values
        valid = list(mem_lens) if mem_lens is not None else [L] * B
        print(path, os.path.getsize(path), "unk", int(unk.sum()), "max weight per step (utterance 0):",
              np.round(wmax[0].numpy(), 3).tolist(), "fp32 vs fp64",
              {k: float(v) for k, v in rec.items() if k.endswith("fp64")})
        for b in range(B):
            if valid[b] > 2 and bool(((wmax[b] >= 2.0 / valid[b]) & (wmax[b] <= 0.999)).any()):
                informative = True
    if not informative:
        raise SystemExit("every step's largest attention weight is < 2 / L or > 0.999: rescale the asr.* synthesis rules")


if __name__ == "__main__":
    main()
