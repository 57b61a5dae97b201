"""Training the whole text aligner on the device: the GroupNorm / dropout kernels of csrc/aligner_cnn_train.hip against
torch and against their unfused pairs, asr.ASRCNN(trainable=True) against the reference's train-mode fixtures
(tests/golden/make_golden_aligner_train.py), determinism, the opt-in interface and TrainStep(train_aligner=True).

Bars.  Kernels against torch: the error against fp64 <= max(2 x torch's own fp32 error against fp64, 1e-4) of the
tensor's max (test_gpu_s2s_train.test_against_torch_restatement's rule).  Outputs against the fixtures:
test_gpu_s2s_train._fwd_bar.  Gradients: test_gpu_train_pred._check_fixture."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import GOLDEN, fill_module
from stts2_mi355x import synth
from test_gpu_s2s_train import _fwd_bar
from test_gpu_train_pred import _check_fixture

pytestmark = pytest.mark.gpu
N_TOKEN = 35
CASES = ("A", "B", "C", "D")
# (B, L, C, G); L = 50 is three row slices of 16, 17 and 17 rows
GN_SHAPES = ((1, 1, 256, 8), (2, 7, 256, 1), (3, 21, 256, 8), (2, 50, 256, 8), (2, 50, 256, 1))
_NETS, _RUNS = {}, {}


def _t(key, shape, std=1.0):
    return torch.from_numpy(synth.normal("altrain:" + key, shape, std)).cuda()


# ------------------------------------------------------------------------------------------- the kernels
def _gn_inputs(B, L, C, G):
    x = _t(f"gn:x:{B}:{L}:{G}", (B, L, C)) + 0.3
    w = 1.0 + 0.3 * _t(f"gn:w:{G}", (C,))
    b = 0.2 * _t(f"gn:b:{G}", (C,))
    gy = _t(f"gn:gy:{B}:{L}:{G}", (B, L, C))
    return x, w, b, gy


def _gn_ours(x, w, b, gy, G, relu, p=0.0, unfused=False):
    from stts2_mi355x import training as Tr
    xs, ws, bs = (t.clone().requires_grad_(True) for t in (x, w, b))
    if unfused:
        y = Tr.dropout(Tr.group_norm_frames(xs, ws, bs, G, relu), p, ref_transpose=True)
    else:
        y = Tr.group_norm_frames(xs, ws, bs, G, relu, p=p, ref_transpose=True)
    y.backward(gy)
    return y.detach(), xs.grad, ws.grad, bs.grad


def _gn_torch(x, w, b, gy, G, relu, dt):
    xs, ws, bs = (t.to(dt).clone().requires_grad_(True) for t in (x, w, b))
    v = F.relu(xs) if relu else xs
    y = F.group_norm(v.transpose(1, 2), G, ws, bs, 1e-5).transpose(1, 2)
    y.backward(gy.to(dt))
    return y.detach(), xs.grad, ws.grad, bs.grad


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("shape", GN_SHAPES, ids=lambda s: "B%d_L%d_C%d_G%d" % s)
def test_groupnorm_against_torch(shape, relu):
    B, L, C, G = shape
    x, w, b, gy = _gn_inputs(B, L, C, G)
    ours = _gn_ours(x, w, b, gy, G, relu)
    r64, r32 = _gn_torch(x, w, b, gy, G, relu, torch.float64), _gn_torch(x, w, b, gy, G, relu, torch.float32)
    for what, a, t64, t32 in zip(("y", "dx", "dw", "db"), ours, r64, r32):
        scale = float(t64.abs().max())
        eo = float((a.double() - t64).abs().max()) / scale
        er = float((t32.double() - t64).abs().max()) / scale
        print(f"groupnorm {shape} relu={relu} {what}: {eo:.2e} (fp32 torch {er:.2e})")
        assert eo <= max(2.0 * er, 1e-4), (what, eo, er)


def test_groupnorm_all_negative_group():
    """Under relu a group whose inputs are all negative is constant 0: variance 0, rstd = 1 / sqrt(eps), y = b and dx
    exactly 0 there."""
    from stts2_mi355x.engine import call
    B, L, C, G = 2, 7, 256, 8
    x, w, b, gy = _gn_inputs(B, L, C, G)
    x[0, :, :32] = -x[0, :, :32].abs() - 0.01
    y, dx, _, _ = _gn_ours(x, w, b, gy, G, True)
    stats = torch.empty(B, G, 2, device="cuda")
    call("stts_groupnorm_fwd_train", x, w, b, B, L, C, G, 1, 0.0, 0, None, torch.empty_like(x), stats,
         ws=("stts_groupnorm_fwd_train_workspace_bytes", B, L, C, G))
    assert float(stats[0, 0, 0]) == 0.0 and float(stats[0, 0, 1]) == float(np.float32(1.0 / np.sqrt(1e-5)))
    assert torch.equal(y[0, :, :32], b[:32].expand(L, 32))
    assert float(dx[0, :, :32].abs().max()) == 0.0 and float(dx[0, :, 32:].abs().max()) > 0.0
    r64 = _gn_torch(x, w, b, gy, G, True, torch.float64)
    assert float((dx.double() - r64[1]).abs().max()) <= 1e-4 * float(r64[1].abs().max())


@pytest.mark.parametrize("masks", [False, True], ids=["seed", "mask"])
@pytest.mark.parametrize("shape", [(3, 21, 256, 8), (2, 50, 256, 1)], ids=lambda s: "B%d_L%d_C%d_G%d" % s)
def test_fused_groupnorm_dropout_is_the_unfused_pair(shape, masks):
    """GroupNorm + dropout in one launch = stts_groupnorm_fwd_train without dropout, then stts_dropout (the same
    seed) or stts_dropout_mask (the same mask), bit for bit, forward and backward."""
    from stts2_mi355x import training as Tr
    B, L, C, G = shape
    x, w, b, gy = _gn_inputs(B, L, C, G)
    out = []
    for unfused in (False, True):
        torch.manual_seed(11)
        Tr.set_dropout_masks(synth.dropout_mask if masks else None)
        try:
            out.append(_gn_ours(x, w, b, gy, G, True, p=0.2, unfused=unfused))
        finally:
            Tr.set_dropout_masks(None)
    for what, a, u in zip(("y", "dx", "dw", "db"), *out):
        assert torch.equal(a, u), what
    kept = float((out[0][0] != 0).float().mean())
    assert 0.7 < kept < 0.9  # (the dropout ran)
    if masks:  # the injected mask is the reference's [B, C, L] layout
        m = torch.from_numpy(synth.dropout_mask(0, (B, C, L), 0.2)).cuda().transpose(1, 2)
        assert torch.equal(out[0][0] != 0, (m != 0) & (_gn_ours(x, w, b, gy, G, True)[0] != 0))


@pytest.mark.parametrize("masks", [False, True], ids=["seed", "mask"])
def test_fused_dropout_add_is_the_unfused_pair(masks):
    from stts2_mi355x import training as Tr
    x, r, gy = _t("da:x", (3, 21, 256)), _t("da:r", (3, 21, 256)), _t("da:gy", (3, 21, 256))
    out = []
    for unfused in (False, True):
        torch.manual_seed(12)
        Tr.set_dropout_masks(synth.dropout_mask if masks else None)
        try:
            xs, rs = x.clone().requires_grad_(True), r.clone().requires_grad_(True)
            y = (rs + Tr.dropout(xs, 0.2, ref_transpose=True)) if unfused else Tr.dropout_add(xs, rs, 0.2,
                                                                                              ref_transpose=True)
            y.backward(gy)
            out.append((y.detach(), xs.grad, rs.grad))
        finally:
            Tr.set_dropout_masks(None)
    for what, a, u in zip(("y", "dx", "dr"), *out):
        assert torch.equal(a, u), what
    assert torch.equal(out[0][2], gy) and 0.7 < float((out[0][1] != 0).float().mean()) < 0.9


def test_counter_draws_keep_four_fifths():
    """The kept fraction of a 256 x 150 tensor at p = 0.2 lies within 4 sigma of 0.8; another seed, another mask."""
    from stts2_mi355x.engine import call
    n = 256 * 150
    x, r = torch.ones(n, device="cuda"), torch.zeros(n, device="cuda")
    ys = []
    for seed in (1234567, 1234568):
        y = torch.empty_like(x)
        call("stts_dropout_add_fwd", x, r, n, 0.2, seed, None, y)
        ys.append(y)
        kept = float((y != 0).double().mean())
        print("kept", kept)
        assert abs(kept - 0.8) <= 4.0 * np.sqrt(0.2 * 0.8 / n)
        assert torch.equal(y[y != 0], torch.full_like(y[y != 0], float(np.float32(1.0) / (np.float32(1.0) - np.float32(0.2)))))
    assert not torch.equal(ys[0], ys[1])


# ------------------------------------------------------------------------------------------- the module
def _net(trainable=True, cfg=(35, 256)):
    from stts2_mi355x.asr import ASRCNN
    key = (trainable, cfg)
    if key not in _NETS:
        _NETS[key] = fill_module(ASRCNN(n_token=cfg[0], token_embedding_dim=cfg[1], trainable=trainable), "asr.").cuda()
    return _NETS[key]


def _case(name):
    fx = np.load(os.path.join(GOLDEN, f"aligner_train_{name}.npz"))
    B, T, L, Tt = int(fx["B"]), int(fx["T"]), int(fx["L"]), int(fx["Tt"])
    mel = np.stack([synth.normal(f"aligner:mel:{b}:{T}", (80, T)) for b in range(B)])
    mask = None
    if fx["mel_lens"][0] >= 0:
        for b, n in enumerate(fx["mel_lens"]):
            mel[b, :, n:] = 0.0
        mask = (torch.arange(L)[None, :] + 1 > (torch.from_numpy(fx["mel_lens"]) // 2)[:, None]).cuda()
    probes = [_t(f"probe:{k}:{B}:{L}:{Tt}", shp) for k, shp in
              (("c", (B, L, N_TOKEN)), ("l", (B, Tt + 1, N_TOKEN)), ("a", (B, Tt + 1, L)))]
    return fx, torch.from_numpy(mel).cuda(), mask, torch.from_numpy(fx["tokens"]).cuda(), \
        torch.from_numpy(fx["unk_mask"]), probes


def _forward_backward(mel, mask, tok, unk, probes, mask_fn=synth.dropout_mask, seed=None):
    from stts2_mi355x import training as Tr
    net = _net().train()
    net.zero_grad(set_to_none=True)
    if seed is not None:
        torch.manual_seed(seed)
    Tr.set_dropout_masks(mask_fn)
    try:
        out = net(mel, mask, tok, unk_mask=unk)
    finally:
        Tr.set_dropout_masks(None)
    sum((o * p).sum() for o, p in zip(out, probes)).backward()
    return [o.detach() for o in out], {k: p.grad.clone() for k, p in net.named_parameters()}


def _run(name):
    """One train-mode forward + backward per case with the fixture's masks, shared by the tests (never modified)."""
    if name not in _RUNS:
        fx, mel, mask, tok, unk, probes = _case(name)
        _RUNS[name] = (fx, mask) + tuple(_forward_backward(mel, mask, tok, unk, probes))
    return _RUNS[name]


@pytest.mark.parametrize("name", CASES)
def test_parity_with_reference(name):
    """Outputs under _fwd_bar, all 142 gradients under _check_fixture, masked frames exactly 0.

    The gradient bar (1e-4 of the module's largest) assumes the 37 ReLUs decide as in the fp64 run: one decision
    taken differently moves a weight gradient by 2e-3 to 1e-2.  The fixtures' mel lengths keep every fp64
    pre-activation at least 1.2e-5 (C) / 4.0e-6 (D) from zero (make_golden_aligner_train.py says how they were
    picked); measured on an MI355X the HIP forward then takes every decision alike and the gradients are within
    3.7e-6 (A), 5.4e-6 (B), 9.3e-6 (C), 6.0e-6 (D) of fp64 per tensor, 2.1e-6 module-normwise at the worst."""
    fx, mask, out, grads = _run(name)
    for k, o in zip(("ctc", "s2s_logit", "attn"), out):
        _fwd_bar(o, fx[k], float(fx[k + "_fp32_vs_fp64"]), f"{name} {k}")
    assert len(grads) == 142
    _check_fixture(grads, fx, f"aligner train {name}")
    if mask is not None:  # masked memory frames: exactly 0 in the alignments
        assert float(out[2][mask[:, None, :].expand_as(out[2])].abs().max()) == 0.0


def test_two_runs_are_bitwise_equal():
    _, _, out1, g1 = _run("C")
    _, mel, mask, tok, unk, probes = _case("C")
    out2, g2 = _forward_backward(mel, mask, tok, unk, probes)
    assert all(torch.equal(a, b) for a, b in zip(out1, out2))
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k


def test_each_batch_row_alone_reproduces_its_outputs():
    """Row b run alone (with row b of the batch's dropout masks) gives row b of the three outputs bit for bit: no
    statistic, slice count or sum order depends on B."""
    _, _, out, _ = _run("C")
    _, mel, mask, tok, unk, probes = _case("C")
    B = mel.shape[0]
    for b in range(B):
        fn = lambda k, shape, p, b=b: synth.dropout_mask(k, (B,) + tuple(shape[1:]), p)[b:b + 1]  # noqa: E731
        row, _ = _forward_backward(mel[b:b + 1], mask[b:b + 1], tok[b:b + 1], unk[b:b + 1],
                                   [p[b:b + 1] for p in probes], mask_fn=fn)
        for k, a, r in zip(("ctc", "s2s_logit", "attn"), out, row):
            assert torch.equal(a[b:b + 1], r), (b, k)


def test_counter_draws_follow_the_seed():
    _, mel, mask, tok, unk, probes = _case("B")
    _, g1 = _forward_backward(mel, mask, tok, unk, probes, mask_fn=None, seed=21)
    _, g2 = _forward_backward(mel, mask, tok, unk, probes, mask_fn=None, seed=21)
    _, g3 = _forward_backward(mel, mask, tok, unk, probes, mask_fn=None, seed=22)
    assert all(torch.equal(g1[k], g2[k]) for k in g1)
    assert any(not torch.equal(g1[k], g3[k]) for k in g1)


def test_interface():
    from stts2_mi355x.asr import ASRCNN
    fx, mel, mask, tok, unk, _ = _case("B")
    tr, df = _net(True).eval(), _net(False).eval()
    a, b = tr(mel, mask, tok, unk_mask=unk), df(mel, mask, tok, unk_mask=unk)
    assert all(torch.equal(x, y) and not x.requires_grad for x, y in zip(a, b))  # eval: the plan, the same bits
    assert torch.equal(tr(mel), df(mel)) and torch.equal(tr.get_feature(mel), df.get_feature(mel))
    tr.train()
    ctc, s2s, attn = tr(mel, mask, tok, unk_mask=unk)
    assert all(t.grad_fn is not None for t in (ctc, s2s, attn))
    assert ctc.shape == (2, 7, N_TOKEN) and s2s.shape == (2, 4, N_TOKEN) and attn.shape == (2, 4, 7)
    only = tr(mel)
    feat = tr.get_feature(mel.unsqueeze(1))
    assert only.shape == ctc.shape and only.grad_fn is not None and feat.shape == (2, 128, 7) and feat.requires_grad
    with pytest.raises(RuntimeError):
        tr(mel.cpu(), None, tok.cpu())
    with pytest.raises(NotImplementedError):
        df.train()(mel, mask, tok)
    with pytest.raises(NotImplementedError):
        ASRCNN().train()(mel)
    df.eval()
    tr.eval()


def test_refusals_by_return_code():
    from stts2_mi355x.engine import lib
    L_ = lib()
    B, L, C, G = 2, 7, 256, 8
    x, w, b, gy = _gn_inputs(B, L, C, G)
    y, stats = torch.empty_like(x), torch.empty(B, G, 2, device="cuda")
    ws = torch.empty(max(L_.stts_groupnorm_fwd_train_workspace_bytes(B, L, C, G),
                         L_.stts_groupnorm_bwd_workspace_bytes(B, L, C, G)), dtype=torch.uint8, device="cuda")
    p = lambda t: t.data_ptr()  # noqa: E731
    fwd = lambda x_=p(x), B_=B, L_n=L, C_=C, G_=G, pr=0.2, nb=ws.numel(): L_.stts_groupnorm_fwd_train(  # noqa: E731
        x_, p(w), p(b), B_, L_n, C_, G_, 1, pr, 5, None, p(y), p(stats), p(ws), nb, None)
    bwd = lambda dy_=p(gy), G_=G, pr=0.2, nb=ws.numel(): L_.stts_groupnorm_bwd(  # noqa: E731
        p(x), p(w), p(stats), dy_, B, L, C, G_, 1, pr, 5, None, p(y), None, None, p(ws), nb, None)
    assert fwd() == 0 and bwd() == 0
    for q in (L_.stts_groupnorm_fwd_train_workspace_bytes, L_.stts_groupnorm_bwd_workspace_bytes):
        assert q(B, L, C, G) > 0
        assert q(0, L, C, G) == q(B, 0, C, G) == q(B, L, 0, G) == q(B, L, C, 0) == q(B, L, C, 7) == -1
    assert fwd(x_=None) == -1 and fwd(B_=0) == -1 and fwd(L_n=0) == -1 and fwd(C_=0) == -1 and fwd(G_=7) == -1
    assert fwd(pr=1.0) == -1 and fwd(pr=-0.1) == -1 and fwd(nb=256) == -4
    assert bwd(dy_=None) == -1 and bwd(G_=7) == -1 and bwd(pr=1.0) == -1 and bwd(nb=256) == -4
    n = x.numel()
    assert L_.stts_dropout_add_fwd(p(x), p(gy), n, 0.2, 5, None, p(y), None) == 0
    assert L_.stts_dropout_add_fwd(None, p(gy), n, 0.2, 5, None, p(y), None) == -1
    assert L_.stts_dropout_add_fwd(p(x), None, n, 0.2, 5, None, p(y), None) == -1
    assert L_.stts_dropout_add_fwd(p(x), p(gy), 0, 0.2, 5, None, p(y), None) == -1
    assert L_.stts_dropout_add_fwd(p(x), p(gy), n, 1.0, 5, None, p(y), None) == -1
    mel, dct, out = torch.zeros(1, 80, 4, device="cuda"), torch.zeros(80, 40, device="cuda"), torch.empty(1, 4, 40, device="cuda")
    assert L_.stts_mfcc_frames(p(mel), p(dct), 1, 80, 4, 40, p(out), None) == 0
    assert L_.stts_mfcc_frames(None, p(dct), 1, 80, 4, 40, p(out), None) == -1
    assert L_.stts_mfcc_frames(p(mel), p(dct), 0, 80, 4, 40, p(out), None) == -1
    assert L_.stts_mfcc_frames(p(mel), p(dct), 1, 80, 0, 40, p(out), None) == -1
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------- the training step
BIG = (178, 512)  # the text encoder's symbol table


def _step(aligner, **kw):
    from helpers import make_decoder, make_duration_modules
    from test_gpu_train_step import _discs
    from stts2_mi355x.models import StyleEncoder
    from stts2_mi355x.trainstep import TrainStep
    te, pp = make_duration_modules()
    dec, _ = make_decoder("hifigan")
    mpd, msd = _discs()
    se = fill_module(StyleEncoder(dim_in=64, style_dim=128, max_conv_dim=512)).cuda().eval()
    return TrainStep(dec.cuda().eval(), mpd.cuda().train(), msd.cuda().train(), predictor=pp.cuda().eval(),
                     style_encoder=se, text_encoder=te.cuda().eval(), text_aligner=aligner, **kw)


def _step_inputs():
    from helpers import duration_inputs
    from test_gpu_train_step import _train_inputs
    T, lengths, frames, ml = 24, (24, 20), (60, 47), 40
    tok, ln, _, _ = duration_inputs(T, lengths)
    B, Tm = len(lengths), 2 * max(frames)
    mels = np.stack([synth.normal(f"ta:mel:{b}:{Tm}", (80, Tm)) for b in range(B)])
    for b, f in enumerate(frames):
        mels[b, :, 2 * f:] = 0.0
    _, _, _, _, wav, noise = _train_inputs(B, ml)
    text = dict(texts=torch.from_numpy(tok).cuda(), input_lengths=torch.from_numpy(ln), mels=torch.from_numpy(mels).cuda(),
                starts=[3, 2], mel_len=ml, mel_input_length=torch.tensor([2 * f for f in frames]),
                unk_mask=torch.from_numpy(synth.hash_u01("ta:unk", B * T).reshape(B, T) < 0.1))
    kw = dict(noise=noise.cuda(), F0_real=torch.from_numpy(synth.normal(f"ta:f0real:{ml}", (B, 2 * ml))).float().abs().cuda() * 200,
              N_real=torch.from_numpy(synth.normal(f"ta:nreal:{ml}", (B, 2 * ml))).float().cuda())
    return text, wav.cuda(), kw


def test_train_step_steps_the_aligner():
    """TrainStep(train_aligner=True): the aligner's gradients are, bit for bit, those of the same composition by hand
    (with the monotonic alignment feeding asr, only loss_mono and loss_s2s reach the aligner), every parameter with a
    gradient moves, and the two returned losses are losses.s2s_loss / mono_loss on the same tensors."""
    from stts2_mi355x import losses
    from stts2_mi355x.align import mask_from_lens, maximum_path
    from stts2_mi355x.asr import ASRCNN
    text, wav, kw = _step_inputs()
    mk = lambda: fill_module(ASRCNN(n_token=BIG[0], token_embedding_dim=BIG[1], trainable=True), "asr.").cuda().train()  # noqa: E731
    net = mk()
    before = {k: p.detach().clone() for k, p in net.named_parameters()}
    step = _step(net, train_aligner=True, capture=True)
    torch.manual_seed(31)
    out = step(None, None, None, None, wav, text=text, **kw)
    got = step.captured["text_aligner"]
    hand = mk()  # the same weights, the same draws: the aligner is the step's first consumer of the generator
    torch.manual_seed(31)
    half = text["mel_input_length"].cuda() // 2
    mask = torch.arange(text["mels"].shape[-1] // 2, device="cuda")[None, :] + 1 > half[:, None]
    _, s2s_pred, attn = hand(text["mels"], mask, text["texts"], unk_mask=text["unk_mask"])
    attn = attn[:, 1:, :].contiguous()
    with torch.no_grad():
        mono = maximum_path(attn.detach(), mask_from_lens(attn, text["input_lengths"], half))
    ls, lm = losses.s2s_loss(s2s_pred, text["texts"], text["input_lengths"]), losses.mono_loss(attn, mono)
    (1.0 * lm + 1.0 * ls).backward()
    assert torch.equal(out["loss_s2s"], ls.detach()) and torch.equal(out["loss_mono"], lm.detach())
    want = {k: p.grad for k, p in hand.named_parameters() if p.grad is not None}
    assert sorted(got) == sorted(want) and len(want) == 142 - 4  # (train.py never reads ppgs: ctc_linear's four stay)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    moved = {k: not torch.equal(before[k], p.detach()) for k, p in net.named_parameters()}
    assert all(moved[k] for k in want), [k for k in want if not moved[k]]
    assert "text_aligner" in step.opt and all(torch.isfinite(v).all() for v in out.values())


def test_train_step_default_is_unchanged():
    """train_aligner=False (the default) returns what a TrainStep built without the keyword returns, bit for bit."""
    text, wav, kw = _step_inputs()
    al = _net(False, BIG).eval()
    outs = []
    for extra in ({}, {"train_aligner": False}):
        torch.manual_seed(32)
        outs.append(_step(al, **extra)(None, None, None, None, wav, text=text, **kw))
    assert sorted(outs[0]) == sorted(outs[1]) and "loss_s2s" not in outs[0]
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k
    assert all(p.grad is None for p in al.parameters())
