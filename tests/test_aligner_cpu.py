"""CPU tests of the text aligner drop-in (stts2_mi355x.asr.ASRCNN <- Modules/ASR/models.py), the alignment search's
host side (stts2_mi355x.align) and what came with them: the state-dict layout, the STTS_KIND_ALIGNER plan's parameter
names, the size queries and refusals, the DCT buffer, the search restatement against brute force.  No GPU compute."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

from mas_ref import brute_force, mas
from stts2_mi355x import engine as E

HERE = os.path.dirname(os.path.abspath(__file__))
CFGS = ((178, 512), (35, 256))  # (n_token, token_embedding_dim): the config's, the constructor's defaults


def _keys(cfg):
    with open(os.path.join(HERE, "golden", "aligner_keys.json")) as f:
        return [(k, tuple(s)) for k, s in json.load(f)["%d_%d" % cfg]]


def _net(cfg):
    from stts2_mi355x.asr import ASRCNN
    return ASRCNN(input_dim=80, hidden_dim=256, n_token=cfg[0], n_layers=6, token_embedding_dim=cfg[1])


def _plan(cfg):
    arr = (ctypes.c_int * len(cfg))(*cfg)
    h = ctypes.c_void_p()
    return E.lib().stts_model_create(E.KIND_ALIGNER, arr, len(cfg), ctypes.byref(h)), h


@pytest.mark.parametrize("cfg", CFGS)
def test_state_dict_is_the_reference_layout(cfg):
    net = _net(cfg)
    ref = _keys(cfg)
    assert len(ref) == 143
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == ref
    assert net.n_token == cfg[0] and net.n_down == 1
    net.load_state_dict({k: torch.zeros(s) for k, s in ref}, strict=True)


def test_constructor_defaults_are_the_reference():
    from stts2_mi355x.asr import ASRCNN
    assert ASRCNN().cfg == [80, 256, 35, 6, 256]


@pytest.mark.parametrize("cfg", CFGS)
def test_plan_names_are_state_dict_keys(cfg):
    rc, h = _plan([80, 256, cfg[0], 6, cfg[1]])
    assert rc == 0
    L = E.lib()
    sd = _net(cfg).state_dict()
    names = [L.stts_param_name(h, i).decode() for i in range(L.stts_param_count(h))]
    assert len(names) == len(set(names)) == 143 and set(names) == set(sd)
    for i, n in enumerate(names):
        assert L.stts_param_numel(h, i) == sd[n].numel(), n
    for dt in (0, 2):
        assert L.stts_packed_bytes(h, dt) > 0
        for B, T, Tt in ((1, 1, 0), (1, 2, 1), (3, 41, 9), (2, 800, 150)):
            a = L.stts_aligner_workspace_bytes(h, dt, B, T, Tt)
            assert a > 0
            assert L.stts_workspace_bytes(h, dt, B, T) == L.stts_aligner_workspace_bytes(h, dt, B, T, 0) <= a
    # bf16 is refused (GroupNorm and the recurrence are fp32), and so are bad sizes
    assert L.stts_workspace_bytes(h, 1, 1, 8) == -2 and L.stts_aligner_workspace_bytes(h, 1, 1, 8, 2) == -2
    assert L.stts_aligner_workspace_bytes(h, 0, 0, 8, 2) == -1 and L.stts_aligner_workspace_bytes(h, 0, 1, 0, 2) == -1
    assert L.stts_aligner_workspace_bytes(h, 0, 1, 8, -1) == -1
    assert L.stts_aligner_workspace_bytes(h, 0, 1, 2 * 4096 + 1, 0) == -1  # L > 4096
    assert L.stts_aligner_workspace_bytes(None, 0, 1, 8, 2) == -1
    # the forward's refusals, before anything is launched
    one = ctypes.c_void_p(1)  # (a non-null pointer that is never read)
    args = (one, None, None, None, 1, 8, 0, None, None, None, None, None, 0, None)
    assert L.stts_aligner_fwd(h, 1, *args) == -2                                     # bf16
    assert L.stts_aligner_fwd(h, 0, None, *args[1:]) == -1                           # no mel
    assert L.stts_aligner_fwd(h, 0, one, None, None, None, 0, 8, 0, *args[7:]) == -1  # B = 0
    assert L.stts_aligner_fwd(h, 0, one, None, one, None, 1, 8, 0, *args[7:]) == -1  # tokens without a length
    assert L.stts_aligner_fwd(h, 0, *args) == -3                                     # parameters not bound
    assert L.stts_aligner_fwd(None, 0, *args) == -1
    L.stts_model_destroy(h)


def test_bad_cfg_rejected():
    for cfg in ([1], [], [80, 256, 178, 6], [40, 256, 178, 6, 512], [80, 512, 178, 6, 512], [80, 256, 3, 6, 512],
                [80, 256, 178, 0, 512], [80, 256, 178, 6, 0], [80, 256, 178, 6, 512, 1]):
        rc, h = _plan(cfg)
        assert rc == -1 and not h.value, cfg


def test_maximum_path_refusals():
    L = E.lib()
    one = ctypes.c_void_p(1)
    ints = lambda *v: (ctypes.c_int * len(v))(*v)  # noqa: E731
    assert L.stts_maximum_path_workspace_bytes(2, 5, 9) >= 2 * 5 * 9 * 5
    assert L.stts_maximum_path_workspace_bytes(0, 5, 9) == -1 and L.stts_maximum_path_workspace_bytes(1, 4097, 5000) == -1
    ok = (one, ints(3, 2), ints(7, 2), 2, 5, 9, one, one, 1 << 20, None)
    for i in (0, 1, 2, 6):  # null pointers
        bad = list(ok)
        bad[i] = None
        assert L.stts_maximum_path(*bad) == -1, i
    assert L.stts_maximum_path(one, ints(3, 2), ints(7, 2), 0, 5, 9, one, one, 1 << 20, None) == -1  # B = 0
    assert L.stts_maximum_path(one, ints(3, 4), ints(7, 3), 2, 5, 9, one, one, 1 << 20, None) == -1  # tx > ty
    assert L.stts_maximum_path(one, ints(0, 2), ints(7, 3), 2, 5, 9, one, one, 1 << 20, None) == -1  # tx < 1
    assert L.stts_maximum_path(one, ints(6, 2), ints(7, 3), 2, 5, 9, one, one, 1 << 20, None) == -1  # tx > Tx
    assert L.stts_maximum_path(one, ints(3, 2), ints(10, 3), 2, 5, 9, one, one, 1 << 20, None) == -1  # ty > Ty
    assert L.stts_maximum_path(*ok[:7], None, 0, None) == -4                                         # no workspace
    from stts2_mi355x.align import mask_from_lens, maximum_path
    v = torch.zeros(2, 5, 9)
    with pytest.raises(ValueError):
        maximum_path(v, mask_from_lens(v, torch.tensor([3, 4]), torch.tensor([7, 3])))
    with pytest.raises(ValueError):
        maximum_path(v, mask_from_lens(v, torch.tensor([0, 2]), torch.tensor([7, 3])))
    with pytest.raises(ValueError):
        maximum_path(v, torch.zeros(2, 5, 8))


def test_train_mode_raises():
    net = _net(CFGS[1])
    x, t = torch.zeros(1, 80, 4), torch.zeros(1, 2, dtype=torch.long)
    for call in (lambda: net.train()(x), lambda: net.train()(x, None, t), lambda: net.train().get_feature(x)):
        with pytest.raises(NotImplementedError):
            call()
    from stts2_mi355x.asr import ASRCNN
    with pytest.raises(NotImplementedError):
        ASRCNN(hidden_dim=128).eval()(x)
    with pytest.raises(IndexError):
        net.eval()(x, None, torch.tensor([[1, 35]]))


def test_forward_refuses_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from stts2_mi355x.align import maximum_path
    with pytest.raises(RuntimeError):
        _net(CFGS[1]).eval()(torch.zeros(1, 80, 4))
    with pytest.raises(RuntimeError):
        maximum_path(torch.zeros(1, 2, 3), torch.ones(1, 2, 3))


def test_dct_mat_is_the_formula():
    d = _net(CFGS[1]).to_mfcc.dct_mat
    assert d.dtype == torch.float32 and tuple(d.shape) == (80, 40)
    want = np.zeros((40, 80))
    for k in range(40):
        for n in range(80):
            want[k, n] = math.cos(math.pi / 80 * (n + 0.5) * k) * (1 / math.sqrt(2) if k == 0 else 1) * math.sqrt(2 / 80)
    # the module evaluates the formula in fp32, as torchaudio does: the cosine's argument reaches pi 39 79.5 / 80 = 122,
    # where two fp32 roundings (pi / 80 (n + 0.5), then x k) move it by up to 2 x 2^-18 = 7.6e-6; x sqrt(2 / 80) = 0.158
    # that is 1.2e-6 on the value, plus the value's own rounding: 4e-6 bounds it
    assert np.abs(d.numpy().T - want).max() < 4e-6
    # orthonormal rows, as 'ortho' promises (80 such terms per entry)
    assert np.abs(d.double().numpy().T @ d.double().numpy() - np.eye(40)).max() < 80 * 4e-6 * 0.158
    from stts2_mi355x import synth
    assert synth.is_fixed_buffer("to_mfcc.dct_mat") and not synth.is_fixed_buffer("init_cnn.conv.weight")


def test_unk_mask_is_the_reference_draw():
    net = _net(CFGS[1])
    t = torch.zeros(3, 50, dtype=torch.long)
    for s in (0, 7):
        torch.manual_seed(s)
        got = net.draw_unk_mask(t)
        torch.manual_seed(s)
        assert got.dtype == torch.bool and torch.equal(got, torch.rand(t.shape) < 0.1)
    assert 0 < int(got.sum()) < 50


def test_search_restatement_finds_the_optimum():
    rng = np.random.default_rng(0)
    for _ in range(200):
        tx = int(rng.integers(1, 5))
        ty = int(rng.integers(tx, 8))
        val = rng.random((tx + 1, ty + 2)).astype(np.float32)  # (a padded batch entry: more rows and columns)
        p = mas(val, tx, ty)
        assert p[:, ty:].sum() == 0 and p[tx:].sum() == 0
        assert (p[:tx, :ty].sum(0) == 1).all() and (p[:tx, :ty].sum(1) >= 1).all()
        assert abs(float((np.float64(val) * p).sum()) - brute_force(val, tx, ty)) <= 1e-5
    # ties: an all-equal matrix keeps a valid path
    p = mas(np.ones((4, 7), np.float32), 4, 7)
    assert (p.sum(0) == 1).all() and (p.sum(1) >= 1).all()


def test_mask_from_lens_shapes():
    from stts2_mi355x.align import mask_from_lens
    attn = torch.zeros(3, 5, 9)
    m = mask_from_lens(attn, torch.tensor([5, 2, 3]), torch.tensor([9, 4, 3]))
    assert m.dtype == torch.bool and tuple(m.shape) == (3, 5, 9)
    assert m.sum(1)[:, 0].tolist() == [5, 2, 3] and m.sum(2)[:, 0].tolist() == [9, 4, 3]
    assert bool(m[1, :2, :4].all()) and int(m[1].sum()) == 8


def test_train_step_keeps_the_aligner_frozen():
    """TrainStep(text_aligner=) builds no optimizer for it (construction needs no device)."""
    from stts2_mi355x.trainstep import TrainStep
    lin = lambda: torch.nn.Linear(2, 2)  # noqa: E731
    step = TrainStep(lin(), lin(), lin(), text_aligner=_net(CFGS[1]).eval())
    assert set(step.opt) == {"decoder", "mpd", "msd"}
    with pytest.raises(ValueError):
        TrainStep(lin(), lin(), lin()).align(torch.zeros(1, 80, 4), torch.tensor([4]), torch.zeros(1, 2), torch.tensor([2]))
