"""CPU tests of the trainable text aligner (asr.ASRCNN(trainable=True), TrainStep(train_aligner=True)): the fixtures
of tests/golden/make_golden_aligner_train.py, the opt-in keyword and the argument checks.  No GPU compute."""
import json
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
N_TOKEN, EMB = 35, 256
# name: (B, T_mel, L, Tt)
CASES = {"A": (1, 2, 1, 1), "B": (2, 14, 7, 3), "C": (3, 41, 21, 9), "D": (2, 300, 150, 5)}


def _keys():
    with open(os.path.join(GOLDEN, "aligner_keys.json")) as f:
        return [(k, tuple(s)) for k, s in json.load(f)["%d_%d" % (N_TOKEN, EMB)]]


@pytest.mark.parametrize("name", sorted(CASES))
def test_fixture_integrity(name):
    """Names, shapes, and the condition the maker asserts: the reference's own fp32 run within 5e-5 (module-normwise,
    half of _check_fixture's cap) of its fp64 run for every tensor, re-read from the stored values."""
    fx = np.load(os.path.join(GOLDEN, f"aligner_train_{name}.npz"))
    B, T, L, Tt = CASES[name]
    assert (int(fx["B"]), int(fx["T"]), int(fx["L"]), int(fx["Tt"])) == (B, T, L, Tt)
    params = [(k, s) for k, s in _keys() if k != "to_mfcc.dct_mat"]
    names = [str(k) for k in fx["names"]]
    assert len(names) == 142 and sorted(names) == sorted(k for k, _ in params)
    assert fx["ctc"].shape == (B, L, N_TOKEN) and fx["ctc"].dtype == np.float32
    assert fx["s2s_logit"].shape == (B, Tt + 1, N_TOKEN) and fx["attn"].shape == (B, Tt + 1, L)
    assert fx["tokens"].shape == fx["unk_mask"].shape == (B, Tt) and fx["text_lens"].shape == (B,)
    ns = fx["f64.idx"].shape[1]
    assert fx["f64.idx"].shape == fx["f64.val"].shape == fx["f32.val"].shape == (142, ns) and 0 < ns <= 256
    numel = dict((k, int(np.prod(s))) for k, s in params)
    for i, k in enumerate(names):
        assert 0 <= fx["f64.idx"][i].min() and fx["f64.idx"][i].max() < numel[k], k
    assert np.isfinite(fx["f64.val"]).all() and np.isfinite(fx["f32.val"]).all()
    gm = float(fx["f64.maxabs"].max())
    # (L = 1: the softmax over one frame leaves the attention's own parameters without a gradient)
    assert gm > 0 and int((fx["f64.maxabs"] > 0).sum()) >= (142 if L > 1 else 130)
    worst = float((np.abs(fx["f32.val"] - fx["f64.val"]).max(axis=1) / gm).max())
    print(f"{name}: fp32 reference module-normwise worst {worst:.2e}")
    assert worst <= 5e-5
    for k in ("ctc", "s2s_logit", "attn"):
        assert 0.0 <= float(fx[k + "_fp32_vs_fp64"]) < 1e-4
    if fx["mel_lens"][0] >= 0:  # masked memory frames: exactly 0 in the alignments
        mask = np.arange(L)[None, :] + 1 > (fx["mel_lens"] // 2)[:, None]
        assert float(np.abs(fx["attn"][np.broadcast_to(mask[:, None, :], fx["attn"].shape)]).max(initial=0.0)) == 0.0


def test_keyword_is_not_part_of_the_state_dict():
    from stts2_mi355x.asr import ASRCNN
    net = ASRCNN(n_token=N_TOKEN, token_embedding_dim=EMB, trainable=True)
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == _keys()
    assert net.trainable and not ASRCNN().trainable
    net.load_state_dict(ASRCNN().state_dict(), strict=True)


def test_train_mode_needs_a_device_tensor():
    """trainable=True allows .train(); a CPU tensor still raises RuntimeError (no compute fallback), for the logits
    and for get_feature."""
    from stts2_mi355x.asr import ASRCNN
    net = ASRCNN(trainable=True).train()
    with pytest.raises(RuntimeError):
        net(torch.zeros(1, 80, 4), None, torch.zeros(1, 2, dtype=torch.long))
    with pytest.raises(RuntimeError):
        net(torch.zeros(1, 80, 4))
    with pytest.raises(RuntimeError):
        net.get_feature(torch.zeros(1, 80, 4))
    with pytest.raises(NotImplementedError):
        ASRCNN(input_dim=64, trainable=True).train()(torch.zeros(1, 64, 4))


def test_train_step_argument_checks():
    from stts2_mi355x.asr import ASRCNN
    from stts2_mi355x.trainstep import TrainStep
    lin = lambda: torch.nn.Linear(2, 2)  # noqa: E731
    with pytest.raises(ValueError):  # a default-built net cannot train
        TrainStep(lin(), lin(), lin(), text_aligner=ASRCNN().eval(), train_aligner=True)
    with pytest.raises(ValueError):
        TrainStep(lin(), lin(), lin(), train_aligner=True)
    with pytest.raises(NotImplementedError):
        TrainStep(lin(), lin(), lin(), text_aligner=ASRCNN(trainable=True).train(), train_aligner=True, graph=True)
    net = ASRCNN(trainable=True).train()
    step = TrainStep(lin(), lin(), lin(), text_aligner=net, train_aligner=True, lr_aligner=3e-4)
    assert set(step.opt) == {"decoder", "mpd", "msd", "text_aligner"}
    assert step.opt["text_aligner"].param_groups[0]["lr"] == 3e-4 and (step.lambda_mono, step.lambda_s2s) == (1.0, 1.0)
    with pytest.raises(ValueError):  # the aligner runs on the text= dict's mels
        step._step(None, None, None, None, torch.zeros(1, 1, 8), None, None, None, None, None, None, None)
    # the default is today's step: no optimizer for the aligner
    assert "text_aligner" not in TrainStep(lin(), lin(), lin(), text_aligner=ASRCNN().eval()).opt
