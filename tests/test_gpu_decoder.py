"""GPU parity: the HIP decoders (through the drop-in Decoder modules and the C-ABI)
against the golden outputs of the reference modules (tests/golden, made by
tests/golden/make_golden.py) on the same formula weights, inputs and noise.

Tolerances (north star: waveform max-abs < 1e-3 vs the reference CPU path, fp32):
  fp32 path: max-abs <= 1e-3 on the final waveform (the reference's own fp32
             reorder floor is <= 1.75e-5);
  bf16 path: bf16 storage + bf16 MFMA is a throughput mode: checked at max-abs <= 5e-2
             and correlation >= 0.99 with the fp32 reference.
"""
import numpy as np
import pytest
import torch

from helpers import decoder_case, golden, make_decoder

pytestmark = pytest.mark.gpu

_DEC = {}


def dec(kind):
    if kind not in _DEC:
        d, _ = make_decoder(kind)
        _DEC[kind] = d.cuda()
    return _DEC[kind]


def run(kind, B, T, dtype, utt0=0, noise=True, seed=0):
    asr, f0, n, s, nz = decoder_case(B, T, utt0)
    d = dec(kind)
    with torch.no_grad():
        out = d(asr.cuda(), f0.cuda(), n.cuda(), s.cuda(), noise=nz.cuda() if noise else None, seed=seed,
                utt_offset=utt0, dtype=dtype)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("kind", ["hifigan", "istftnet"])
@pytest.mark.parametrize("T,B", [(4, 1), (4, 2), (16, 2), (40, 1)])
def test_decoder_fp32_matches_reference(kind, T, B):
    out = run(kind, B, T, "fp32")
    ref = golden(f"{kind}_T{T}_B{B}")["out"]
    assert out.shape == ref.shape
    err = np.abs(out - ref).max()
    assert err < 1e-3, f"{kind} T={T} B={B}: max-abs {err}"


@pytest.mark.parametrize("kind", ["hifigan", "istftnet"])
def test_decoder_fp32_10s_matches_reference(kind):
    """config 2 (iSTFTNet) / HiFi-GAN, B=1, 10-s utterance: waveform max-abs < 1e-3."""
    out = run(kind, 1, 400, "fp32")
    ref = golden(f"{kind}_T400_B1")["out"]
    err = np.abs(out - ref).max()
    print(f"{kind} 10 s fp32 max-abs err {err:.3e}")
    assert err < 1e-3


@pytest.mark.parametrize("kind", ["hifigan", "istftnet"])
@pytest.mark.parametrize("T,B", [(16, 2), (400, 1)])
def test_decoder_bf16_close_to_reference(kind, T, B):
    out = run(kind, B, T, "bf16")
    ref = golden(f"{kind}_T{T}_B{B}")["out"]
    err = np.abs(out - ref).max()
    corr = np.corrcoef(out.ravel(), ref.ravel())[0, 1]
    print(f"{kind} T={T} bf16 max-abs {err:.3e} corr {corr:.6f}")
    assert corr > 0.99 and err < 5e-2 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_device_rng_is_shard_invariant(dtype):
    """Noise drawn on the device is keyed by the GLOBAL utterance id: a batch of 3 equals
    three single-utterance calls at utt_offset 0, 1, 2 (bit-exact) -> rank-count invariant."""
    T = 8
    asr, f0, n, s, _ = decoder_case(3, T)
    d = dec("hifigan")
    with torch.no_grad():
        full = d(asr.cuda(), f0.cuda(), n.cuda(), s.cuda(), noise=None, seed=7, utt_offset=0, dtype=dtype).cpu()
        parts = [d(asr[i:i + 1].cuda(), f0[i:i + 1].cuda(), n[i:i + 1].cuda(), s[i:i + 1].cuda(), noise=None,
                   seed=7, utt_offset=i, dtype=dtype).cpu() for i in range(3)]
    assert torch.equal(full, torch.cat(parts))
    # and a different seed changes the waveform
    with torch.no_grad():
        other = d(asr.cuda(), f0.cuda(), n.cuda(), s.cuda(), noise=None, seed=8, dtype=dtype).cpu()
    assert not torch.equal(full, other)


@pytest.mark.parametrize("kind,B,T,dtype", [("hifigan", 2, 16, "fp32"), ("hifigan", 4, 64, "fp32"),
                                             ("hifigan", 4, 64, "bf16"), ("hifigan", 3, 48, "bf16x3"),
                                             ("istftnet", 3, 48, "fp32"), ("istftnet", 3, 48, "bf16")])
def test_decoder_deterministic_repeat(kind, B, T, dtype):
    """Repeat decodes are bitwise equal: the InstanceNorm statistics are fixed-point integer sums (order-free
    atomics, csrc/common.h ST_W), the LDS partials have one writer per word, split-K and the other reductions
    run in a fixed order."""
    a = run(kind, B, T, dtype)
    b = run(kind, B, T, dtype)
    assert np.array_equal(a, b), np.abs(a - b).max()


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "bf16x3"])
def test_nan_utterance_stays_isolated(dtype):
    """A NaN in one utterance's input makes that utterance's InstanceNorm statistics NaN (the fixed-point entry's
    poison mark, csrc/common.h ST_POISON) and its output NaN, as the reference's InstanceNorm does; the other
    utterances of the batch are bitwise the same as in a clean batch (statistics are per utterance and channel)."""
    asr, f0, n, s, nz = decoder_case(3, 16)
    d = dec("hifigan")
    bad = asr.clone()
    bad[1, 7, 5] = float("nan")
    with torch.no_grad():
        clean = d(asr.cuda(), f0.cuda(), n.cuda(), s.cuda(), noise=nz.cuda(), dtype=dtype).cpu()
        out = d(bad.cuda(), f0.cuda(), n.cuda(), s.cuda(), noise=nz.cuda(), dtype=dtype).cpu()
    assert torch.isnan(out[1]).all()
    assert torch.equal(out[0], clean[0]) and torch.equal(out[2], clean[2])


@pytest.mark.parametrize("B,T", [(2, 40), (4, 64)])
def test_big64_bf16_decoder_ab(B, T):
    """bf16 C = 64 resblock convs on the bigconv2 engine with 128-frame wave slices (STTS_OPT_BIG64 bit 2) against
    resconv: the same bf16 model, different fp32 accumulation order (and bf16 rounding of intermediates)."""
    from stts2_mi355x import engine as E
    try:
        E.set_option(E.OPT_BIG64, 0)
        ref = run("hifigan", B, T, "bf16")
        E.set_option(E.OPT_BIG64, 2)
        out = run("hifigan", B, T, "bf16")
    finally:
        E.reset_options()
    corr = np.corrcoef(out.ravel(), ref.ravel())[0, 1]
    err = np.abs(out - ref).max()
    print(f"big64 bf16 A/B B={B} T={T}: max-abs {err:.3e} corr {corr:.7f}")
    assert corr > 0.9995 and err < 5e-2


def test_resconv_engine_decoder_ab():
    """bf16 HiFi-GAN decode with the resblock engine on and off: both are the same bf16 model;
    they differ only by fp32 accumulation order (and bf16 rounding of intermediates)."""
    from stts2_mi355x import engine as E
    try:
        E.set_option(E.OPT_RESCONV, 0)
        ref = run("hifigan", 2, 40, "bf16")
        E.set_option(E.OPT_RESCONV, 1)
        out = run("hifigan", 2, 40, "bf16")
    finally:
        E.reset_options()
    corr = np.corrcoef(out.ravel(), ref.ravel())[0, 1]
    err = np.abs(out - ref).max()
    print(f"resconv A/B: max-abs {err:.3e} corr {corr:.7f}")
    assert corr > 0.9995 and err < 5e-2


@pytest.mark.parametrize("dtype,tol", [("fp32", 1e-5), ("bf16", 2e-2)])
def test_head_engine_ab(dtype, tol):
    """HiFi-GAN output head (Snake -> conv_post -> tanh) on the streaming head.hip kernel against the
    igemm engine running the same launch.  fp32: both exact fp32, differing by summation order
    (tol 1e-5).  bf16: the igemm rounds the Snake outputs to bf16 for its MFMA operands, the head
    keeps them fp32, so the two differ by that rounding (tol 2e-2 on a +-1 waveform); the head's
    own accuracy is the golden test above (fp32 max-abs < 1e-3 vs the reference)."""
    from stts2_mi355x import engine as E
    try:
        E.set_option(E.OPT_HEAD, 0)
        ref = run("hifigan", 2, 40, dtype)
        E.set_option(E.OPT_HEAD, 1)
        E.profile_enable(True)
        out = run("hifigan", 2, 40, dtype)
        kernels = {r["kernel"] for r in E.profile_launches()}
    finally:
        E.profile_enable(False)
        E.reset_options()
    assert "k_conv_post" in kernels
    err = np.abs(out - ref).max()
    print(f"head A/B {dtype}: max-abs {err:.3e}")
    assert err < tol


@pytest.mark.parametrize("B,T", [(1, 400), (2, 40)])
def test_pw_split_decoder_ab(B, T):
    """bf16 HiFi-GAN decode at small batch with the short-conv engine (its split-K path serves the
    front-end k3 convs and the 1x1 shortcuts: fp32 slice partials summed in slice order) on and off
    (STTS_OPT_PW 0 = conv1d_igemm).  Same bf16 model, different summation order."""
    from stts2_mi355x import engine as E
    try:
        E.set_option(E.OPT_PW, 0)
        ref = run("hifigan", B, T, "bf16")
        E.set_option(E.OPT_PW, 1)
        E.set_option(E.OPT_SPLITK, 1)
        out = run("hifigan", B, T, "bf16")
        out2 = run("hifigan", B, T, "bf16")
    finally:
        E.reset_options()
    corr = np.corrcoef(out.ravel(), ref.ravel())[0, 1]
    err = np.abs(out - ref).max()
    print(f"pw split-K A/B B={B} T={T}: max-abs {err:.3e} corr {corr:.7f}")
    assert corr > 0.9995 and err < 5e-2
    assert np.array_equal(out, out2)  # deterministic (fixed slice order, no atomics on the outputs)


# ---------------------------------------------------------------- config 3 (BASELINE configs[2])
_CFG3 = {}


def _cfg3_batch():
    """B = 32 ten-second utterances (T = 400 asr frames), formula inputs and formula noise
    (utterance 0 is exactly the hifigan_T400_B1 golden case)."""
    if not _CFG3:
        _CFG3["case"] = decoder_case(32, 400)
    return _CFG3["case"]


def _decode(case, dtype, sl=slice(None)):
    asr, f0, n, s, nz = (t[sl] for t in case)
    d = dec("hifigan")
    with torch.no_grad():
        out = d(asr.cuda(), f0.cuda(), n.cuda(), s.cuda(), noise=nz.cuda(), dtype=dtype)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_config3_fp32_batch32_pinned():
    """Config 3's batch (B = 32 x 10 s) on the production path (default options: one statistics slot,
    full persistent grids, multi-GB workspace offsets) in fp32: utterance 0 equals the reference golden
    within the north-star 1e-3, and every utterance equals its own B = 1 decode within 1e-5.  (The
    statistics are order-free fixed-point sums, so the batch and B = 1 paths differ only where B = 1
    routes launches to other engines: split-K front-end convs, 4-wave tiles, statistics slots.)"""
    case = _cfg3_batch()
    out = _decode(case, "fp32")
    assert out.shape == (32, 1, 240000)
    err0 = np.abs(out[0] - golden("hifigan_T400_B1")["out"][0]).max()
    print(f"config 3 fp32 utterance 0 vs reference golden: {err0:.3e}")
    assert err0 < 1e-3
    worst = 0.0
    for i in range(32):
        one = _decode(case, "fp32", slice(i, i + 1))
        worst = max(worst, float(np.abs(out[i] - one[0]).max()))
    print(f"config 3 fp32: max over utterances of |B=32 - B=1| = {worst:.3e}")
    assert worst < 1e-5
    _CFG3["fp32"] = out


def test_config3_bf16_batch32_shipped_mode():
    """The headline mode (bf16 storage + bf16 MFMA, B = 32 x 10 s, production options) against the
    fp32 decode of the same batch: the measured 10-s max-abs is reported and bounded."""
    case = _cfg3_batch()
    ref = _CFG3.get("fp32")
    if ref is None:
        ref = _decode(case, "fp32")
    out = _decode(case, "bf16")
    err = np.abs(out - ref).reshape(32, -1).max(1)
    corr = min(np.corrcoef(out[i].ravel(), ref[i].ravel())[0, 1] for i in range(32))
    rms = float(np.sqrt(((out - ref) ** 2).mean()))
    print(f"config 3 bf16 vs fp32: max-abs {err.max():.3e} (median over utterances {np.median(err):.3e}), "
          f"rms {rms:.3e}, min corr {corr:.6f}")
    assert corr > 0.999 and err.max() < 5e-2
    # utterance 0 against the reference golden as well
    g = golden("hifigan_T400_B1")["out"][0]
    print(f"config 3 bf16 utterance 0 vs reference golden: {np.abs(out[0] - g).max():.3e}")


@pytest.mark.parametrize("dtype", ["bf16", "fp32", "bf16x3"])
def test_config4_rank_shard_bitwise(dtype):
    """Config 4 (BASELINE configs[3]: 256 utterances sharded 8-way, 32 per rank) on one GPU: a B = 64 x 10 s decode with
    device-RNG noise equals, bit for bit, the two B = 32 decodes that two ranks would run on its halves (utt_offset 0 and
    32).  What makes it hold: the noise is keyed by the global utterance id, the InstanceNorm totals are
    order-free fixed-point sums, and for batches of 32 k utterances every persistent conv launch splits its tiles into
    utterance-relative ranges (STTS_OPT_SEGPART, kernels.h tile_range), so each workgroup's fp32 partial statistics
    cover the same frames whatever the batch size."""
    asr, f0, n, s, _ = decoder_case(64, 400)
    d = dec("hifigan")

    def go(sl, off):
        with torch.no_grad():
            out = d(asr[sl].cuda(), f0[sl].cuda(), n[sl].cuda(), s[sl].cuda(), noise=None, seed=1234,
                    utt_offset=off, dtype=dtype)
        torch.cuda.synchronize()
        return out.cpu()

    full = go(slice(0, 64), 0)
    lo = go(slice(0, 32), 0)
    hi = go(slice(32, 64), 32)
    assert full.shape == (64, 1, 240000)
    assert torch.isfinite(full).all()
    assert torch.equal(full[:32], lo), (full[:32] - lo).abs().max().item()
    assert torch.equal(full[32:], hi), (full[32:] - hi).abs().max().item()


def test_config4_every_rank_count_bitwise():
    """The whole config-4 job in the headline mode (bf16, B = 256 x 10 s, device-RNG noise) decodes the same bits on
    1, 2, 4 and 8 ranks: the B = 256 decode equals every rank's shard decode (256 / W utterances at utt_offset
    r 256 / W) for W = 2, 4, 8."""
    asr, f0, n, s, _ = decoder_case(256, 400)
    d = dec("hifigan")

    def go(a, b):
        with torch.no_grad():
            out = d(asr[a:b].cuda(), f0[a:b].cuda(), n[a:b].cuda(), s[a:b].cuda(), noise=None, seed=99, utt_offset=a,
                    dtype="bf16")
        torch.cuda.synchronize()
        return out.cpu()

    full = go(0, 256)
    assert torch.isfinite(full).all()
    for W in (2, 4, 8):
        per = 256 // W
        for r in range(W):
            part = go(r * per, (r + 1) * per)
            assert torch.equal(full[r * per:(r + 1) * per], part), (W, r)


@pytest.mark.parametrize("cap", [100, 37])
def test_batch32_grid_cap_bitwise(cap):
    """B = 32 (config 3 / a config-4 rank): the statistics launches split into utterance-relative segments whose count
    comes from the full grid, so capping the grid (STTS_OPT_GRID_CAP: several segments per workgroup, the segmented
    kernel instantiations) moves work between workgroups but not a single output bit (device-RNG noise, bf16)."""
    from stts2_mi355x import engine as E
    asr, f0, n, s, _ = decoder_case(32, 40)
    d = dec("hifigan")

    def go():
        with torch.no_grad():
            out = d(asr.cuda(), f0.cuda(), n.cuda(), s.cuda(), noise=None, seed=7, dtype="bf16")
        torch.cuda.synchronize()
        return out.cpu()

    try:
        ref = go()
        E.set_option(E.OPT_GRID_CAP, cap)
        out = go()
    finally:
        E.reset_options()
    assert torch.isfinite(ref).all()
    assert torch.equal(out, ref), (out - ref).abs().max().item()


def test_default_noise_follows_torch_rng():
    """Decoder.forward without noise / seed draws its noise key from torch's default generator, as the
    reference's randn_like draws (hifigan.py:213): successive calls differ, and torch.manual_seed
    makes a call reproducible."""
    asr, f0, n, s, _ = decoder_case(1, 8)
    d = dec("hifigan")
    args = (asr.cuda(), f0.cuda(), n.cuda(), s.cuda())
    with torch.no_grad():
        torch.manual_seed(11)
        a = d(*args).cpu()
        b = d(*args).cpu()
        torch.manual_seed(11)
        c = d(*args).cpu()
    assert not torch.equal(a, b)
    assert torch.equal(a, c)


def test_inplace_weight_update_repacks():
    """An in-place parameter update (its _version moves) makes the packed weights stale: the next
    forward repacks, so the output follows the new weights; invalidate() covers .data writes."""
    from helpers import make_decoder
    d, _ = make_decoder("hifigan")
    d = d.cuda()
    asr, f0, n, s, nz = (t.cuda() for t in decoder_case(1, 8))
    with torch.no_grad():
        a = d(asr, f0, n, s, noise=nz).cpu()
        d.generator.conv_post.bias.add_(0.25)  # tanh(x + 0.25) != tanh(x)
        b = d(asr, f0, n, s, noise=nz).cpu()
        d.generator.conv_post.bias.data.sub_(0.25)  # invisible to the version counter
        d.invalidate()
        c = d(asr, f0, n, s, noise=nz).cpu()
    assert (b - a).abs().max() > 1e-3
    assert (a - c).abs().max() < 1e-5  # ((x + 0.25) - 0.25 is not x in every bit: the bias itself moved)
