"""GPU parity: the text aligner (asr.ASRCNN on the HIP plan) against the reference's golden outputs
(tests/golden/make_golden_aligner.py), the monotonic alignment search on the device against its CPU restatement
(tests/mas_ref.py, bitwise), and the training step computing its own alignments.

Bars.  fp32 / bf16x3: max|out - ref| / max(1, max|ref|) <= max(1e-4 / 2e-4 (the stack bars of test_gpu_pitch.py),
4 x the fixture's own fp32-vs-fp64 difference of that output).  The search: the path is equal bit for bit."""
import numpy as np
import pytest
import torch

from helpers import fill_module, golden
from mas_ref import mas_batch
from stts2_mi355x import synth

pytestmark = pytest.mark.gpu

BIG, DEFAULT = (178, 512), (35, 256)
# (B, T_mel, T_text, mel lengths or None = no padding mask, cfg): tests/golden/make_golden_aligner.py
CASES = (
    (1, 2, 1, (2,), BIG),                # L = 1: softmax over one frame, the location conv all padding
    (2, 14, 3, (14, 6), DEFAULT),        # a masked tail (weights exactly 0 there); the constructor's default sizes
    (3, 41, 9, (41, 26, 33), BIG),       # odd T_mel, L = 21
    (2, 150, 40, None, BIG),             # L = 75: crosses a wave; interior and both borders of the 63-tap conv
    (1, 300, 70, (300,), BIG),           # L = 150: multi-wave softmax, 71 steps of fp32 feedback
)
IDS = [f"B{c[0]}_T{c[1]}_Tt{c[2]}" for c in CASES]
_NETS, _RUNS = {}, {}


def _net(cfg):
    from stts2_mi355x.asr import ASRCNN
    if cfg not in _NETS:
        net = ASRCNN(input_dim=80, hidden_dim=256, n_token=cfg[0], n_layers=6, token_embedding_dim=cfg[1])
        _NETS[cfg] = fill_module(net, "asr.").eval().cuda()
    return _NETS[cfg]


def _inputs(B, T, Tt, mel_lens):
    fx = golden(f"aligner_B{B}_T{T}_Tt{Tt}")
    mel = np.stack([synth.normal(f"aligner:mel:{b}:{T}", (80, T)) for b in range(B)])
    mask = None
    if mel_lens is not None:
        for b, n in enumerate(mel_lens):
            mel[b, :, n:] = 0.0
        mask = (torch.arange((T + 1) // 2)[None, :] + 1 > (torch.tensor(mel_lens) // 2)[:, None]).cuda()
    return fx, torch.from_numpy(mel).cuda(), mask, torch.from_numpy(fx["tokens"]).cuda(), torch.from_numpy(fx["unk_mask"])


def _run(case, dtype):
    """One forward per (case, dtype), shared by the tests that read it (never modified)."""
    if (case, dtype) not in _RUNS:
        B, T, Tt, mel_lens, cfg = case
        fx, mel, mask, tok, unk = _inputs(B, T, Tt, mel_lens)
        _RUNS[(case, dtype)] = (fx, mask) + tuple(_net(cfg)(mel, mask, tok, dtype=dtype, unk_mask=unk))
    return _RUNS[(case, dtype)]


def _err(out, ref):
    return float(np.abs(out - ref).max()) / max(1.0, float(np.abs(ref).max()))


@pytest.mark.parametrize("dtype", ["fp32", "bf16x3"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_aligner(case, dtype):
    B, T, Tt, mel_lens, cfg = case
    fx, mask, ctc, s2s, attn = _run(case, dtype)
    L = (T + 1) // 2
    assert ctc.shape == (B, L, cfg[0]) and s2s.shape == (B, Tt + 1, cfg[0]) and attn.shape == (B, Tt + 1, L)
    for k, out in (("ctc", ctc), ("s2s_logit", s2s), ("attn", attn)):
        bar = max({"fp32": 1e-4, "bf16x3": 2e-4}[dtype], 4.0 * float(fx[k + "_fp32_vs_fp64"]))
        e = _err(out.cpu().numpy(), fx[k])
        print(f"aligner B={B} T={T} Tt={Tt} {dtype} {k}: {e:.3e} (bar {bar:.1e}, ref absmax {np.abs(fx[k]).max():.3f}, "
              f"fixture fp32 vs fp64 {float(fx[k + '_fp32_vs_fp64']):.2e})")
        assert e <= bar, (k, e, bar)
    if mask is not None:  # the padded frames' weights are exactly 0, every step sums to 1
        assert float(attn[mask[:, None, :].expand_as(attn)].abs().max() if mask.any() else 0.0) == 0.0
    assert float((attn.sum(-1) - 1).abs().max()) < 1e-5


def test_bf16_is_refused():
    B, T, Tt, mel_lens, cfg = CASES[1]
    _, mel, mask, tok, unk = _inputs(B, T, Tt, mel_lens)
    with pytest.raises(ValueError):
        _net(cfg)(mel, mask, tok, dtype="bf16", unk_mask=unk)


def test_ctc_alone_and_feature():
    """Without text_input forward returns ctc_logit alone (the same bits); get_feature is the projection output."""
    case = CASES[2]
    B, T, Tt, mel_lens, cfg = case
    _, mel, mask, tok, unk = _inputs(B, T, Tt, mel_lens)
    net = _net(cfg)
    ctc = net(mel)
    assert torch.equal(ctc, _run(case, "fp32")[2])
    feat = net.get_feature(mel.unsqueeze(1))
    assert feat.shape == (B, 128, (T + 1) // 2)
    lin = net.ctc_linear
    ref = lin[2].linear_layer(torch.relu(lin[0].linear_layer(feat.transpose(1, 2))))  # torch on the HIP feature
    assert float((ref - ctc).abs().max()) <= 1e-4 * max(1.0, float(ctc.abs().max()))


def test_batch_invariance_fp32():
    """No cross-utterance state, no atomics: the rows of a B = 3 call are the bits of three B = 1 calls."""
    case = CASES[2]
    B, T, Tt, mel_lens, cfg = case
    _, mel, mask, tok, unk = _inputs(B, T, Tt, mel_lens)
    _, _, ctc, s2s, attn = _run(case, "fp32")
    for b in range(B):
        one = _net(cfg)(mel[b:b + 1], mask[b:b + 1], tok[b:b + 1], unk_mask=unk[b:b + 1])
        for full, o in zip((ctc, s2s, attn), one):
            assert torch.equal(o[0], full[b]), b


def test_null_output_pointers_leave_the_others_bitwise():
    case = CASES[1]
    B, T, Tt, mel_lens, cfg = case
    _, mel, mask, tok, unk = _inputs(B, T, Tt, mel_lens)
    eng = _net(cfg).engine("fp32")
    ctc, s2s, attn, feat = eng.forward(mel, mask, tok, unk, feature=True)
    for keep in ("ctc", "s2s", "attn", "feature"):
        got = eng.forward(mel, mask, tok, unk, **{k: k == keep for k in ("ctc", "s2s", "attn", "feature")})
        for name, a, b in zip(("ctc", "s2s", "attn", "feature"), (ctc, s2s, attn, feat), got):
            assert (b is None) == (name != keep), (keep, name)
            if b is not None:
                assert torch.equal(a, b), (keep, name)


def test_parameter_write_makes_the_pack_stale():
    B, T, Tt, mel_lens, cfg = CASES[1]
    from stts2_mi355x.asr import ASRCNN
    net = fill_module(ASRCNN(n_token=cfg[0], token_embedding_dim=cfg[1]), "asr.").eval().cuda()
    _, mel, mask, tok, unk = _inputs(B, T, Tt, mel_lens)
    a = net(mel, mask, tok, unk_mask=unk)
    eng = net._engine
    with torch.no_grad():
        net.asr_s2s.attention_layer.query_layer.linear_layer.weight.mul_(1.5)
    b = net(mel, mask, tok, unk_mask=unk)
    assert net._engine is not eng and torch.equal(a[0], b[0]) and not torch.equal(a[2], b[2])


def test_default_unk_mask_follows_the_seed():
    B, T, Tt, mel_lens, cfg = CASES[3]
    _, mel, mask, tok, _ = _inputs(B, T, Tt, mel_lens)
    net = _net(cfg)
    torch.manual_seed(3)
    a = net(mel, mask, tok)
    torch.manual_seed(3)
    drawn = torch.rand(tok.shape) < 0.1
    assert drawn.any()
    b = net(mel, mask, tok, unk_mask=drawn)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------- alignment search
def _search(value, tx, ty):
    from stts2_mi355x.align import mask_from_lens, maximum_path
    v = torch.from_numpy(value).cuda()
    path = maximum_path(v, mask_from_lens(v, torch.tensor(tx), torch.tensor(ty)))
    assert path.dtype == v.dtype and path.device == v.device and path.shape == v.shape
    return path.cpu().numpy()


def _check_path(path, value, tx, ty):
    assert np.array_equal(path.astype(np.int32), mas_batch(value, tx, ty))
    for b in range(len(path)):
        p = path[b]
        assert set(np.unique(p)) <= {0.0, 1.0}
        assert p[tx[b]:].sum() == 0 and p[:, ty[b]:].sum() == 0
        assert (p[:tx[b], :ty[b]].sum(0) == 1).all() and (p[:tx[b], :ty[b]].sum(1) >= 1).all()


SEARCH = {
    "random": ((7, 19), [(7, 19)]),
    "tx_is_1": ((3, 9), [(1, 9)]),
    "tx_is_ty": ((6, 6), [(6, 6)]),
    "ty_is_tx_plus_1": ((6, 7), [(6, 7)]),
    "padded_batch": ((12, 40), [(12, 40), (5, 17), (9, 9)]),
    "wave_boundary": ((65, 257), [(65, 257)]),       # rows cross a wave, columns cross 256
    "block_boundary": ((130, 300), [(130, 300)]),
    "rows_beyond_the_block": ((300, 310), [(300, 310), (257, 258)]),  # lanes loop over x
}


@pytest.mark.parametrize("name", list(SEARCH))
def test_maximum_path_bitwise(name):
    (Tx, Ty), lens = SEARCH[name]
    tx, ty = [a for a, _ in lens], [b for _, b in lens]
    value = np.stack([synth.normal(f"mas:{name}:{b}", (Tx, Ty)) for b in range(len(lens))])
    _check_path(_search(value, tx, ty), value, tx, ty)


def test_maximum_path_ties_and_dtype():
    value = np.ones((2, 9, 21), np.float32)
    tx, ty = [9, 4], [21, 11]
    _check_path(_search(value, tx, ty), value, tx, ty)
    from stts2_mi355x.align import mask_from_lens, maximum_path
    v = torch.from_numpy(synth.normal("mas:half", (1, 5, 11))).cuda().half()
    p = maximum_path(v, mask_from_lens(v, torch.tensor([5]), torch.tensor([11])))
    assert p.dtype == torch.float16
    assert np.array_equal(p.float().cpu().numpy().astype(np.int32), mas_batch(v.float().cpu().numpy(), [5], [11]))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_maximum_path_on_the_aligner_attention(case):
    B, T, Tt, mel_lens, cfg = case
    fx, mask, _, _, attn = _run(case, "fp32")
    value = attn[:, 1:, :].contiguous().cpu().numpy()
    tx = [int(v) for v in fx["text_lens"]]
    ty = [n // 2 for n in mel_lens] if mel_lens is not None else [(T + 1) // 2] * B
    _check_path(_search(value, tx, ty), value, tx, ty)


# ---------------------------------------------------------------------------------------------- the training step
def _step_modules():
    from helpers import make_decoder, make_duration_modules
    from test_gpu_train_step import _discs
    from stts2_mi355x.models import StyleEncoder
    from stts2_mi355x.trainstep import TrainStep
    te, pp = make_duration_modules()
    dec, _ = make_decoder("hifigan")
    mpd, msd = _discs()
    se = fill_module(StyleEncoder(dim_in=64, style_dim=128, max_conv_dim=512)).cuda().eval()
    return TrainStep(dec.cuda().eval(), mpd.cuda().train(), msd.cuda().train(), predictor=pp.cuda().eval(),
                     style_encoder=se, text_encoder=te.cuda().eval(), text_aligner=_net(BIG))


def test_train_step_aligns():
    """TrainStep(text_aligner=).align is train.py:203-214 by hand, and a step whose text= dict leaves the alignments
    out equals, bit for bit, the step given align's outputs."""
    from helpers import duration_inputs
    from test_gpu_train_step import _train_inputs
    from stts2_mi355x.align import mask_from_lens, maximum_path
    T, lengths, frames, ml = 24, (24, 20), (60, 47), 40
    tok, ln, _, _ = duration_inputs(T, lengths)
    B, Tm = len(lengths), 2 * max(frames)
    mels = np.stack([synth.normal(f"ta:mel:{b}:{Tm}", (80, Tm)) for b in range(B)])
    for b, f in enumerate(frames):
        mels[b, :, 2 * f:] = 0.0
    mels = torch.from_numpy(mels).cuda()
    mel_len = torch.tensor([2 * f for f in frames])
    texts, lens = torch.from_numpy(tok).cuda(), torch.from_numpy(ln)
    unk = torch.from_numpy(synth.hash_u01("ta:unk", B * T).reshape(B, T) < 0.1)
    _, _, _, _, wav, noise = _train_inputs(B, ml)
    F0_real = torch.from_numpy(synth.normal(f"ta:f0real:{ml}", (B, 2 * ml))).float().abs().cuda() * 200
    N_real = torch.from_numpy(synth.normal(f"ta:nreal:{ml}", (B, 2 * ml))).float().cuda()
    step = _step_modules()
    attn, mono = step.align(mels, mel_len, texts, lens, unk_mask=unk)
    assert attn.shape == mono.shape == (B, T, Tm // 2)
    with torch.no_grad():  # by hand
        mask = (torch.arange(Tm // 2)[None, :] + 1 > (mel_len // 2)[:, None]).cuda()
        _, _, a = step.text_aligner(mels, mask, texts, unk_mask=unk)
        a = a[:, 1:, :].contiguous()
        m = maximum_path(a, mask_from_lens(a, lens, mel_len // 2))
    assert torch.equal(attn, a) and torch.equal(mono, m)
    assert mono.sum(-1)[0].min() >= 1 and float(mono[1, lengths[1]:].abs().max()) == 0.0
    common = dict(texts=texts, input_lengths=lens, mels=mels, starts=[3, 2], mel_len=ml)
    run = lambda st, text: st(None, None, None, None, wav.cuda(), noise=noise.cuda(), F0_real=F0_real,  # noqa: E731
                              N_real=N_real, text=text)
    out_a = run(step, dict(common, mel_input_length=mel_len, unk_mask=unk))
    out_b = run(_step_modules(), dict(common, attn=mono, attn_mono=mono))
    for k in out_a:
        assert torch.equal(out_a[k], out_b[k]), k
    assert all(p.grad is None for p in step.text_aligner.parameters()) and "text_aligner" not in step.opt
