"""What of the S2S decoder's training path can be checked without a device: the ABI rows and the header, the module's
keys, the fixtures (tests/golden/make_golden_s2s_train.py) and the torch restatement (tests/s2s_ref.py) against them."""
import json
import os
import re

import numpy as np
import pytest
import torch

from helpers import GOLDEN, fill_module
from s2s_ref import KEYS, s2s_forward
from stts2_mi355x import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("A", "B", "Bdrop", "C", "D")
ENTRIES = ("stts_s2s_save_bytes", "stts_s2s_fwd_train_workspace_bytes", "stts_s2s_fwd_train",
           "stts_s2s_bwd_workspace_bytes", "stts_s2s_bwd", "stts_s2s_loss_workspace_bytes", "stts_s2s_loss",
           "stts_mono_loss")
N_TOKEN, D = 35, 128


def test_entries_in_table_and_header():
    from stts2_mi355x.abi import SIGNATURES
    with open(os.path.join(ROOT, "include", "stts2_train.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in ENTRIES:
        assert name in SIGNATURES, name
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/stts2_train.h"
        assert len(m.group(1).split(",")) == len(SIGNATURES[name][0]), name
    assert "#define STTS_S2S_BWD_MAX_L" in text


def test_module_keys_are_the_references():
    from stts2_mi355x.asr import ASRS2S
    assert tuple(k for k, _ in ASRS2S(embedding_dim=256, hidden_dim=128, n_token=35).named_parameters()) == KEYS
    with open(os.path.join(GOLDEN, "aligner_keys.json")) as f:
        ref = [k[len("asr_s2s."):] for k, _ in json.load(f)["35_256"] if k.startswith("asr_s2s.")]
    assert tuple(ref) == KEYS


def _case(name):
    fx = np.load(os.path.join(GOLDEN, f"s2s_train_{name}.npz"))
    B, L, Tt = int(fx["B"]), int(fx["L"]), int(fx["Tt"])
    mem = torch.from_numpy(np.stack([synth.normal(f"s2s:mem:{b}:{L}", (L, D)) for b in range(B)]))
    mask = None
    if fx["mem_lens"][0] >= 0:
        mask = torch.from_numpy(np.arange(L)[None, :] >= fx["mem_lens"][:, None])
    return fx, B, L, Tt, mem, mask


@pytest.mark.parametrize("name", CASES)
def test_fixture_is_self_consistent(name):
    fx, B, L, Tt, mem, mask = _case(name)
    assert fx["hidden"].shape == (B, Tt + 1, D) and fx["logit"].shape == (B, Tt + 1, N_TOKEN)
    assert fx["attn"].shape == (B, Tt + 1, L) and fx["tokens"].shape == fx["unk_mask"].shape == (B, Tt)
    assert np.abs(fx["attn"].sum(-1) - 1.0).max() <= 1e-5
    if mask is not None:
        assert np.abs(fx["attn"][np.broadcast_to(mask.numpy()[:, None, :], fx["attn"].shape)]).max() == 0.0
    names = [str(k) for k in fx["names"]]
    assert names[:14] == list(KEYS) and names[14] == "dmemory"
    assert fx["f64.val"].shape == fx["f32.val"].shape == fx["f64.idx"].shape == (15, 256)
    gm = float(fx["f64.maxabs"].max())
    for i, k in enumerate(names):  # the fp32 reference itself inside the bars the device path is held to
        scale = max(float(fx["f64.maxabs"][i]), 1e-3 * gm)
        assert np.abs(fx["f32.val"][i] - fx["f64.val"][i]).max() / scale <= 1e-4, k
        assert float(fx["f64.maxabs"][i]) > 0.0 or L == 1, k  # (one frame: the weight is 1 whatever the energies)
    for k in ("hidden", "logit", "attn"):
        assert float(fx[k + "_fp32_vs_fp64"]) <= 2.5e-5


@pytest.mark.parametrize("name", CASES)
def test_restatement_agrees_with_fixture(name):
    from stts2_mi355x.asr import ASRCNN
    fx, B, L, Tt, mem, mask = _case(name)
    net = fill_module(ASRCNN(), "asr.").asr_s2s.double()
    ps = [p for _, p in net.named_parameters()]
    m = mem.double().requires_grad_(True)
    scale = None
    if bool(fx["train"]):
        scale = torch.from_numpy(synth.dropout_mask(0, (B, Tt + 1, D), 0.5)).double() / 0.5
    out = s2s_forward(ps, m, mask, torch.from_numpy(fx["tokens"]), torch.from_numpy(fx["unk_mask"]), scale)
    probes = [torch.from_numpy(synth.normal(f"s2s:probe:{k}:{B}:{L}:{Tt}", tuple(o.shape))).double()
              for k, o in zip("hla", out)]
    sum((o * p).sum() for o, p in zip(out, probes)).backward()
    for k, o in zip(("hidden", "logit", "attn"), out):
        assert float((o.detach() - torch.from_numpy(fx[k]).double()).abs().max()) <= max(1e-6, 4 * float(
            fx[k + "_fp32_vs_fp64"])), k
    grads = {**{k: p.grad for k, p in zip(KEYS, ps)}, "dmemory": m.grad}
    for i, k in enumerate(str(n) for n in fx["names"]):
        g = grads[k].reshape(-1)[torch.from_numpy(fx["f64.idx"][i])].numpy()
        assert np.abs(g - fx["f64.val"][i]).max() <= 1e-9 * max(1.0, float(fx["f64.maxabs"][i])), k


def test_build_models_text_aligner():
    from stts2_mi355x.inference import build_models
    from test_loader import CONFIG
    cfg = dict(CONFIG, model_params=dict(CONFIG["model_params"], ASR_params={
        "input_dim": 80, "hidden_dim": 256, "n_layers": 6, "token_embedding_dim": 512}))
    models = build_models(cfg, text_aligner=True)
    with open(os.path.join(GOLDEN, "aligner_keys.json")) as f:
        ref = [k for k, _ in json.load(f)["178_512"]]
    assert list(models["text_aligner"].state_dict()) == ref
    assert models["text_aligner"].asr_s2s.embedding.weight.shape[1] == 512
    assert "text_aligner" not in build_models(cfg)
