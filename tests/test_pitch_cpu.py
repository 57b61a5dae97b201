"""CPU tests of the pitch extractor drop-in (stts2_mi355x.jdc.JDCNet <- Modules/JDC/model.py) and what came with it:
the state-dict layout, the STTS_KIND_PITCH plan's parameter names, the refusals, the synthesis rules and
build_models' new keyword.  No GPU compute here."""
import ctypes
import json
import os
import zlib

import numpy as np
import pytest
import torch

from stts2_mi355x import engine as E
from stts2_mi355x import synth

HERE = os.path.dirname(os.path.abspath(__file__))

# the state-dict entries JDCNet.forward never reads (model.py:102-137): the detector branch and BatchNorm's counters
NOT_IN_PLAN = ("detector_conv.", "bilstm_detector.", "detector.")


def _keys():
    with open(os.path.join(HERE, "golden", "pitch_keys.json")) as f:
        return [(k, tuple(s)) for k, s in json.load(f)]


def _plan(cfg):
    L = E.lib()
    arr = (ctypes.c_int * len(cfg))(*cfg)
    h = ctypes.c_void_p()
    return L.stts_model_create(E.KIND_PITCH, arr, len(cfg), ctypes.byref(h)), h


def test_state_dict_is_the_reference_layout():
    from stts2_mi355x.jdc import JDCNet
    net = JDCNet(num_class=1, seq_len=192)
    sd = net.state_dict()
    ref = _keys()
    assert len(ref) == 77
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == ref
    assert sum(p.numel() for p in net.parameters()) == 5248067  # SURVEY §4 (component 16)
    # the reference's own entry loads strictly
    net.load_state_dict({k: torch.zeros(s) if "num_batches" not in k else torch.zeros(s, dtype=torch.long)
                         for k, s in ref}, strict=True)


@pytest.mark.parametrize("num_class", [1, 5])
def test_plan_names_are_state_dict_keys(num_class):
    from stts2_mi355x.jdc import JDCNet
    rc, h = _plan([num_class])
    assert rc == 0
    L = E.lib()
    sd = JDCNet(num_class=num_class, seq_len=192).state_dict()
    names = [L.stts_param_name(h, i).decode() for i in range(L.stts_param_count(h))]
    assert len(names) == len(set(names)) == 53
    expect = {k for k in sd if not k.startswith(NOT_IN_PLAN) and not k.endswith("num_batches_tracked")}
    assert set(names) == expect
    for i, n in enumerate(names):
        assert L.stts_param_numel(h, i) == sd[n].numel(), n
    for dt in (0, 1, 2):
        assert L.stts_packed_bytes(h, dt) > 0
        for B, T in ((1, 1), (3, 130), (2, 310)):
            ws = L.stts_workspace_bytes(h, dt, B, T)
            off = L.stts_pitch_error_offset(h, dt, B, T)
            assert 0 < off and off % 8 == 0 and off + 8 <= ws, (dt, B, T, off, ws)
    assert L.stts_workspace_bytes(h, 0, 1, 0) < 0 and L.stts_pitch_error_offset(h, 0, 0, 4) < 0
    # forward without parameters / packed weights fails loudly
    assert L.stts_pitch_fwd(h, 0, None, 1, 4, None, None, None, None, 0, None) < 0
    L.stts_model_destroy(h)


def test_bad_cfg_rejected():
    for cfg in ([0], [-3], [1, 192], []):
        rc, _ = _plan(cfg)
        assert rc == -1, cfg  # STTS_EINVAL
    assert E.lib().stts_log_norm(None, 1, 80, 4, -4.0, 4.0, None, None) == -1


def test_train_mode_and_other_slopes_raise():
    from stts2_mi355x.jdc import JDCNet
    x = torch.zeros(1, 1, 80, 4)
    with pytest.raises(NotImplementedError):
        JDCNet(num_class=1, seq_len=192).train()(x)
    with pytest.raises(NotImplementedError):
        JDCNet(num_class=1, seq_len=192, leaky_relu_slope=0.2).eval()(x)


def test_forward_refuses_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from stts2_mi355x.jdc import JDCNet
    from stts2_mi355x.losses import log_norm
    with pytest.raises(RuntimeError):
        JDCNet(num_class=1, seq_len=192).eval()(torch.zeros(1, 1, 80, 4))
    with pytest.raises(RuntimeError):
        log_norm(torch.zeros(1, 1, 80, 4))


def test_log_norm_serves_only_the_reference_call():
    from stts2_mi355x.losses import log_norm
    for x, kw in ((torch.zeros(2, 80, 4), {}), (torch.zeros(2, 1, 80, 4), {"dim": 3}), (torch.zeros(2, 2, 80, 4), {})):
        with pytest.raises(NotImplementedError):
            log_norm(x, **kw)


# (key, shape, crc32 of the float32 bytes, bits of element 0): one key per synthesis rule that existed before the
# BatchNorm rules, computed with the synth.py of the commit before them
OLD_RULES = (
    ("generator.ups.0.weight_v", (8, 4, 3), 0x72c9e7c9, 0xbc696fea),
    ("decode.0.conv1.parametrizations.weight.original1", (4, 4, 3), 0xd5177c03, 0x3f044e83),
    ("generator.ups.0.weight_g", (8, 1, 1), 0xbbeaa013, 0x3f9586fb),
    ("encode.conv1.parametrizations.weight.original0", (6, 1, 1), 0xd4e373a5, 0x3f4f0fa2),
    ("generator.resblocks.0.alpha1.0", (1, 8, 1), 0xa05e71bc, 0x3f2ef666),
    ("generator.alphas.1", (1, 8, 1), 0x3421bf5e, 0x3f5d99f4),
    ("encode.norm1.fc.weight", (16, 128), 0x93534656, 0x3ce62d91),
    ("encode.norm1.fc.bias", (16,), 0x7a90540a, 0xbd4399af),
    ("generator.m_source.l_linear.weight", (1, 9), 0xebc06f9e, 0x3e167daa),
    ("pp.lstm.weight_ih_l0", (32, 12), 0xff055b1c, 0xbcd9eab4),
    ("pp.lstm.bias_hh_l0_reverse", (32,), 0xded413df, 0xbdc5767a),
    ("te.embedding.weight", (5, 7), 0xb8032048, 0x4029544e),
    ("generator.noise_convs.0.weight", (4, 1, 6), 0x6c572128, 0xbebfcebe),
    ("F0_proj.weight", (1, 8, 1), 0x461b7b03, 0x3e30a2cf),
    ("shared.0.weight", (4, 1, 3, 3), 0x19116417, 0x3d022d5b),
    ("shared.0.bias", (4,), 0x9fb02585, 0xbbdfa952),
    ("generator.convnext.0.gamma", (8,), 0x3b9b67f8, 0x3e0cf457),
    ("generator.final_layer_norm.weight", (8,), 0x5d6f5b74, 0x3f8ae708),
    ("te.cnn.0.1.gamma", (8,), 0x879332b2, 0x3f4dfc07),
    ("te.cnn.0.1.beta", (8,), 0x5b2dc442, 0x3d7b3b13),
)


def test_synth_rules_for_batchnorm_leave_old_keys_alone():
    for key, shape, crc, first in OLD_RULES:
        v = synth.synth_param(key, shape)
        assert v.dtype == np.float32 and v.shape == shape
        assert zlib.crc32(v.tobytes()) == crc and int(v.ravel()[:1].view(np.uint32)[0]) == first, key
    w = synth.synth_param("jdc.conv_block.1.weight", (64,))
    m = synth.synth_param("jdc.conv_block.1.running_mean", (64,))
    var = synth.synth_param("jdc.conv_block.1.running_var", (64,))
    assert 0.8 <= w.min() and w.max() <= 1.2 and -0.1 <= m.min() and m.max() <= 0.1
    assert 0.5 <= var.min() and var.max() <= 1.5
    assert synth.is_fixed_buffer("conv_block.1.num_batches_tracked")
    assert not synth.is_fixed_buffer("conv_block.1.running_var")


def test_build_models_keyword():
    from test_loader import CONFIG
    from stts2_mi355x.inference import build_models
    from stts2_mi355x.jdc import JDCNet
    assert set(build_models(CONFIG)) == {"decoder", "predictor", "text_encoder", "style_encoder"}
    cfg = dict(CONFIG, model_params=dict(CONFIG["model_params"], JDC_params={"num_class": 1, "seq_len": 192}))
    m = build_models(cfg, pitch_extractor=True)
    assert set(m) == {"decoder", "predictor", "text_encoder", "style_encoder", "pitch_extractor"}
    pe = m["pitch_extractor"]
    assert isinstance(pe, JDCNet) and pe.num_class == 1 and pe.seq_len == 192


def test_train_step_keeps_the_extractor_frozen():
    """TrainStep(pitch_extractor=) builds no optimizer for it (construction needs no device)."""
    from stts2_mi355x.jdc import JDCNet
    from stts2_mi355x.trainstep import TrainStep
    lin = lambda: torch.nn.Linear(2, 2)  # noqa: E731
    step = TrainStep(lin(), lin(), lin(), pitch_extractor=JDCNet(num_class=1, seq_len=192).eval())
    assert set(step.opt) == {"decoder", "mpd", "msd"}
    with pytest.raises(ValueError):
        TrainStep(lin(), lin(), lin()).targets(torch.zeros(1, 80, 4))
