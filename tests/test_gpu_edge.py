"""GPU edge cases of the decoder path, checked against the CPU oracle (oracle/stts_oracle.py)
computed in the test on the same formula weights, inputs and noise:

  * odd and tiny lengths (T = 2, 3, 7 asr frames): every generator stage ends in a partial
    tile, the front-end has a single tile, and the stride-2 F0/N convs see odd lengths;
  * batch composition: an utterance decodes the same alone and inside a batch (per-utterance
    InstanceNorm statistics never mix);
  * host-side validation and device placement of the drop-in Decoder.

Tolerances: fp32 max-abs <= 1e-3 (north star); bf16 correlation >= 0.99 with the fp32 oracle.
"""

import numpy as np
import pytest
import torch

from helpers import golden, decoder_case, make_decoder
from oracle import stts_oracle as orc

pytestmark = pytest.mark.gpu

_DEC = {}


def dec(kind):
    if kind not in _DEC:
        d, cfg = make_decoder(kind)
        sd = {k: v.detach().clone() for k, v in d.state_dict().items()}
        _DEC[kind] = (d.cuda(), sd, cfg)
    return _DEC[kind]


def oracle(kind, asr, f0, n, s, noise):
    _, sd, cfg = dec(kind)
    fn = orc.decoder_hifigan if kind == "hifigan" else orc.decoder_istft
    with torch.no_grad():
        return fn(asr, f0, n, s, sd, cfg, noise).numpy()


def gpu(kind, asr, f0, n, s, noise, dtype):
    d, _, _ = dec(kind)
    with torch.no_grad():
        out = d(asr.cuda(), f0.cuda(), n.cuda(), s.cuda(), noise=noise.cuda(), dtype=dtype)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("kind", ["hifigan", "istftnet"])
@pytest.mark.parametrize("T", [2, 3, 7])
def test_odd_lengths_fp32(kind, T):
    case = decoder_case(3, T, utt0=5)
    ref = oracle(kind, *case)
    out = gpu(kind, *case, "fp32")
    assert out.shape == ref.shape == (3, 1, 600 * T)
    err = np.abs(out - ref).max()
    tol = 1e-3
    if T == 2:
        # every InstanceNorm averages two frames and near-equal pairs make the forward ill-conditioned.
        # The bound is pinned by the REFERENCE's own conditioning (tests/golden/make_golden_edge.py):
        # its output moves by spread_perturbed under a 1e-6 relative weight perturbation and by
        # spread_fp64 against a float64 run (hifigan 3.4e-3 / 4.5e-3, istftnet 8.9e-5 / 1.8e-4);
        # the GPU result must sit within 10x that of the reference's own output.
        g = golden(f"{kind}_T2_B3_edge")
        spread = max(float(g["spread_perturbed"]), float(g["spread_fp64"]))
        tol = max(1e-3, 10 * spread)
        err_ref = np.abs(out - g["out"]).max()
        print(f"{kind} T=2: max-abs vs reference {err_ref:.3e} (tol {tol:.2e}), vs oracle {err:.3e}")
        assert err_ref < tol, f"{kind} T=2: max-abs vs reference {err_ref}"
    assert err < tol, f"{kind} T={T}: max-abs {err}"


@pytest.mark.parametrize("kind", ["hifigan", "istftnet"])
def test_odd_length_bf16(kind):
    case = decoder_case(2, 7, utt0=9)
    ref = oracle(kind, *case)
    out = gpu(kind, *case, "bf16")
    corr = np.corrcoef(out.ravel(), ref.ravel())[0, 1]
    assert corr > 0.99 and np.abs(out - ref).max() < 5e-2 * max(1.0, np.abs(ref).max()), corr


@pytest.mark.parametrize("dtype,tol", [("fp32", 1e-4), ("bf16", 2e-2)])
def test_batch_composition(dtype, tol):
    """Utterance 1 of a batch of 3 equals the same utterance decoded alone (same noise)."""
    asr, f0, n, s, noise = decoder_case(3, 8, utt0=2)
    full = gpu("hifigan", asr, f0, n, s, noise, dtype)
    one = gpu("hifigan", asr[1:2], f0[1:2], n[1:2], s[1:2], noise[1:2], dtype)
    assert np.abs(full[1:2] - one).max() < tol


def test_cpu_inputs_come_back_on_cpu():
    d, _, _ = dec("hifigan")
    asr, f0, n, s, noise = decoder_case(1, 2)
    with torch.no_grad():
        out = d(asr, f0, n, s, noise=noise, dtype="fp32")
    assert out.device.type == "cpu" and tuple(out.shape) == (1, 1, 1200)


def test_shape_validation():
    d, _, _ = dec("hifigan")
    asr, f0, n, s, noise = (t.cuda() for t in decoder_case(2, 4))
    with torch.no_grad():
        with pytest.raises(ValueError):
            d(asr, f0[:, :-1], n, s, noise=noise)          # F0 must be [B, 2T]
        with pytest.raises(ValueError):
            d(asr[:, :-1], f0, n, s, noise=noise)          # asr must have dim_in channels
        with pytest.raises(ValueError):
            d(asr, f0, n, s, noise=noise[:, :-1])          # noise must be [B, 600T, 9]
        with pytest.raises(ValueError):                    # one frame: the reference's
            d(asr[..., :1], f0[:, :2], n[:, :2], s)        # InstanceNorm1d raises too


@pytest.mark.parametrize("dtype,B", [("fp32", 1), ("bf16", 1), ("bf16", 3)])
def test_stats_slots_do_not_change_results(dtype, B):
    """Small-batch statistics spreading (STTS_OPT_STATS_SLOTS, slots folded after each launch) only
    reorders fp64 sums: outputs with 1, 16 and 64 slots agree (fp32 to 1e-5; bf16 to 1e-2, the
    rounding of a bf16 activation may flip) and fp32 still matches the oracle."""
    from stts2_mi355x import engine as E
    d, sd, cfg = dec("hifigan")
    asr, f0, n, s, noise = decoder_case(B, 7)
    outs = []
    try:
        for slots in (1, 16, 64):
            E.set_option(E.OPT_STATS_SLOTS, slots)
            with torch.no_grad():
                outs.append(d(asr.cuda(), f0.cuda(), n.cuda(), s.cuda(), noise=noise.cuda(), dtype=dtype).cpu())
    finally:
        E.set_option(E.OPT_STATS_SLOTS, 0)
    tol = 1e-5 if dtype == "fp32" else 1e-2
    assert (outs[0] - outs[1]).abs().max().item() < tol
    assert (outs[0] - outs[2]).abs().max().item() < tol
    if dtype == "fp32":
        with torch.no_grad():
            ref = orc.decoder_hifigan(asr, f0, n, s, sd, cfg, noise)
        assert (outs[1] - ref).abs().max().item() < 1e-3


def test_small_tiles_do_not_change_results():
    """STTS_OPT_SMALL_TILES (64 x 128 implicit-GEMM tiles for few-tile launches) vs the 128 x 128 fp32
    tiles: same sums per output, so the fp32 decoder output agrees to 1e-5."""
    from stts2_mi355x import engine as E
    d, sd, cfg = dec("istftnet")
    asr, f0, n, s, noise = decoder_case(1, 9)
    outs = []
    try:
        for on in (1, 0):
            E.set_option(6, on)
            with torch.no_grad():
                outs.append(d(asr.cuda(), f0.cuda(), n.cuda(), s.cuda(), noise=noise.cuda(), dtype="fp32").cpu())
    finally:
        E.set_option(6, 1)
    assert (outs[0] - outs[1]).abs().max().item() < 1e-5


def _fxsum(parts, mode):
    """The total of `parts` through one fixed-point statistics entry (stts_test_fxsum: each part added by its own
    lane with integer atomics, then read back once)."""
    from stts2_mi355x import engine as E
    L = E.lib()
    t = torch.as_tensor(parts, dtype=torch.float32 if mode == 0 else torch.float64).cuda()
    entry = torch.zeros(4, dtype=torch.float64, device="cuda")
    out = torch.zeros(1, dtype=torch.float64, device="cuda")
    rc = L.stts_test_fxsum(mode, t.data_ptr(), t.numel(), entry.data_ptr(), out.data_ptr(),
                           torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return float(out.item())


@pytest.mark.parametrize("mode", [0, 1])
def test_fixed_point_statistics_range(mode):
    """The InstanceNorm statistics entries (csrc/common.h fx_add / fx_get): an in-range total is exact to the entry's
    2^-48 resolution; a part or a total beyond the 2^45 range reads back as NaN (the reference's InstanceNorm then
    gives NaN / inf as well), never as a silently wrapped, wrong mean or variance."""
    rng = np.random.default_rng(3)
    p = rng.standard_normal(50_000).astype(np.float32) * 100.0
    tot = _fxsum(p, mode)
    assert abs(tot - float(p.astype(np.float64).sum())) < 1e-6
    # every part in range (2^40 each), the total 64 x 2^40 = 2^46 beyond it: NaN, not a wrapped value
    assert np.isnan(_fxsum(np.full(64, 2.0 ** 40), mode))
    # 2^40 x 1,024 = 2^50: past the int64 word's 2^47 wrap point, far from a multiple of 2^48: NaN too
    assert np.isnan(_fxsum(np.full(1024, 2.0 ** 40) * np.where(np.arange(1024) % 5 == 0, 1.0, 0.75), mode))
    # a single out-of-range part, and a NaN part, poison the entry
    assert np.isnan(_fxsum(np.array([1.0, 2.0 ** 46, -2.0 ** 46]), mode))
    assert np.isnan(_fxsum(np.array([1.0, np.nan, 3.0]), mode))
    # negative totals near the edge of the range are still read back
    q = np.full(16, -(2.0 ** 40))
    assert _fxsum(q, mode) == -(2.0 ** 44)
