"""GPU parity of the assembled training step (BASELINE config 5) through the C-ABI:

* each new HIP autograd piece (Snake with learned alpha, tanh, branch sums, the source module, the
  train-mode smoothing, the MSD time expansion, |STFT|, the GAN loss terms incl. TPRLS, the
  multi-resolution mel loss, AdamW) against torch autograd of the oracle / torch in fp64 on the CPU;
* the whole decoder's parameter and input gradients, and the MPD / MSD gradients, against autograd
  through the oracle (fp32, CPU), which tests/test_train_oracle_cpu.py pins bit-exactly to the
  reference's own autograd;
* one D + G step (train.py:267-327 with AdamW) against the reference fixture tests/golden/
  train_step_B2_T8.npz (made by tests/golden/make_golden_train.py from the reference modules);
* the full config-5 shape (B = 2 x 93,000 samples) against the oracle's step.

Tolerances: fp32 gradients within 1e-4 of the tensor's max |g| (floored at 1e-3 of the largest max |g| of
the module: parameters whose true gradient is ~0, e.g. a conv bias feeding an InstanceNorm, carry only
rounding noise); the mel loss is parity-unpinned upstream (torchaudio is absent: DESIGN §6e).
"""
import copy
import random

import numpy as np
import pytest
import torch

from helpers import HIFI_CFG, fill_module, golden, make_decoder
from oracle import stts_oracle as orc
from stts2_mi355x import synth

pytestmark = pytest.mark.gpu


def _rel(a, b, floor=0.0):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), floor, 1e-30))


def _waves(B, L, seed):
    return torch.from_numpy(synth.waves(B, L, seed))


def _train_inputs(B, T):
    asr, f0, n, s = (torch.from_numpy(a) for a in synth.decoder_inputs(B, T, tag="train"))
    L = 600 * T
    return asr, f0, n, s, _waves(B, L, 7), torch.from_numpy(synth.source_noise(B, L, tag="train_noise"))


def _discs():
    from stts2_mi355x.discriminators import MultiPeriodDiscriminator, MultiResSpecDiscriminator
    return fill_module(MultiPeriodDiscriminator(), "mpd."), fill_module(MultiResSpecDiscriminator(), "msd.")


def _sd(m):
    return {k: v.detach().clone().cpu() for k, v in m.state_dict().items()}


def _check_grads(ours, ref, tol=1e-4, what="", floor_frac=1e-3):
    gmax = max(float(g.abs().max()) for g in ref.values() if g is not None)
    worst = (0.0, None)
    for k, g in ref.items():
        if g is None:
            assert ours.get(k) is None, k
            continue
        assert ours.get(k) is not None, f"{what}: no gradient for {k}"
        e = _rel(ours[k], g, floor=floor_frac * gmax)
        worst = max(worst, (e, k))
    print(f"{what}: worst gradient error {worst[0]:.2e} ({worst[1]}), {len(ref)} tensors, max |g| {gmax:.3e}")
    assert worst[0] < tol, worst


def _sd64(sd):
    return {k: v.double() for k, v in sd.items()}


def _check3(ours, r32, r64, what, slack=2.0, abs_tol=1e-4, norm_tol=None):
    """Gradients vs the oracle's fp64 autograd (the truth), next to the reference's own fp32 error: the
    reference in fp32 is itself 1.6e-4 (decoder) to 3.3e-4 (MSD) of max |g| away from fp64 at T = 8
    (tests/golden/make_golden_train.py's case), so 'as close as the reference' means
    err(ours, fp64) <= max(slack * err(fp32 reference, fp64), abs_tol) per tensor (same floor as _check_grads)."""
    gmax = max(float(g.abs().max()) for g in r64.values() if g is not None)
    worst, worst_ref = (0.0, None), (0.0, None)
    for k, g in r64.items():
        if g is None:
            continue
        assert ours.get(k) is not None, f"{what}: no gradient for {k}"
        eo = _rel(ours[k], g, floor=1e-3 * gmax)
        er = _rel(r32[k], g, floor=1e-3 * gmax)
        worst, worst_ref = max(worst, (eo, k)), max(worst_ref, (er, k))
        assert eo <= max(slack * er, abs_tol), (k, eo, er)
        if norm_tol is not None:  # error relative to the module's largest |g|
            assert _rel(ours[k], g, floor=gmax) <= norm_tol, (k, "normwise", _rel(ours[k], g, floor=gmax))
    print(f"{what}: vs fp64, ours worst {worst[0]:.2e} ({worst[1]}), fp32 reference worst {worst_ref[0]:.2e} "
          f"({worst_ref[1]}), {len(r64)} tensors")


# ------------------------------------------------------------------ the pieces
def test_snake_tanh_sum():
    from stts2_mi355x import training as T
    torch.manual_seed(0)
    x = torch.randn(2, 300, 48, dtype=torch.float64)
    a = (0.5 + torch.rand(1, 48, 1, dtype=torch.float64))
    gy = torch.randn(2, 300, 48, dtype=torch.float64)
    xd, ad = x.float().cuda().requires_grad_(True), a.float().cuda().requires_grad_(True)
    y = T.snake(xd, ad)
    y.backward(gy.float().cuda())
    xr, ar = x.clone().requires_grad_(True), a.clone().requires_grad_(True)
    yr = orc.snake(xr.transpose(1, 2), ar).transpose(1, 2)
    yr.backward(gy)
    assert _rel(y.detach(), yr.detach()) < 1e-6
    assert _rel(xd.grad, xr.grad) < 1e-5 and _rel(ad.grad, ar.grad) < 1e-5
    # tanh, sum / average
    t = torch.randn(1000, device="cuda", requires_grad=True)
    T.tanh(t).sum().backward()
    tr = t.detach().cpu().double().requires_grad_(True)
    torch.tanh(tr).sum().backward()
    assert _rel(t.grad, tr.grad) < 1e-6
    xs = [torch.randn(5, 7, device="cuda", requires_grad=True) for _ in range(3)]
    out = T.sum_div(xs, 3)
    c = [v.detach().cpu() for v in xs]
    assert torch.equal(out.detach().cpu(), ((c[0] + c[1]) + c[2]) / 3)  # the reference's CPU rounding (a true division)
    out.sum().backward()
    assert all(torch.allclose(v.grad, torch.full_like(v, 1 / 3)) for v in xs)


def test_native_calls_run_on_the_current_side_stream():
    """engine.call appends torch's *current* stream: inside torch.cuda.stream(side), _TanhFn's forward and backward
    read an input that `side` writes only after a few ms of queued work, so a launch on a stream not ordered after
    `side` would read the zeros the tensor held before (the null stream does order itself after `side` on this
    runtime: substituting it still passes).  Bar 1e-6 absolute against fp64: |tanh| < 1 and 0 < tanh' <= 1, a few fp32 ulps
    (6e-8 each) of tanhf, and 2 |y| times that again for 1 - y^2."""
    from stts2_mi355x import training as T
    vals = torch.tensor([-1.5, 0.25, 3.0])
    vals_d = vals.cuda()
    side = torch.cuda.Stream()
    x = torch.zeros(3, device="cuda")
    busy = torch.zeros(1 << 26, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(40):
            busy.add_(1.0)
        x.copy_(vals_d)  # (device to device: the host does not wait for `side` here)
        xg = x.requires_grad_(True)
        y = T.tanh(xg)
        y.sum().backward()
    side.synchronize()
    ref = vals.double().requires_grad_(True)
    yr = torch.tanh(ref)
    yr.sum().backward()
    assert (y.detach().cpu().double() - yr.detach()).abs().max() < 1e-6
    assert (xg.grad.cpu().double() - ref.grad).abs().max() < 1e-6


@pytest.mark.parametrize("k", [3, 7, 15])
def test_box_smooth(k):
    from stts2_mi355x import training as T
    torch.manual_seed(k)
    x = torch.randn(3, 50, dtype=torch.float64)
    g = torch.randn(3, 50, dtype=torch.float64)
    xd = x.float().cuda().requires_grad_(True)
    y = T.box_smooth(xd, k)
    y.backward(g.float().cuda())
    xr = x.clone().requires_grad_(True)
    yr, _ = orc.train_smooth(xr, xr, k, 0)
    yr.backward(g)
    assert _rel(y.detach(), yr.detach()) < 1e-6 and _rel(xd.grad, xr.grad) < 1e-6


def test_source_module_grads():
    from stts2_mi355x import training as T
    B, n = 2, 16
    _, f0, _, _ = synth.decoder_inputs(B, n // 2, tag="train")
    f0 = torch.from_numpy(f0)
    L = 300 * n
    noise = torch.from_numpy(synth.source_noise(B, L, tag="src"))
    W = torch.randn(1, 9) * 0.3
    b = torch.randn(1) * 0.1
    gy = torch.randn(B, L)
    Wd, bd = W.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    har = T._SourceFn.apply(f0.cuda(), Wd, bd, noise.cuda(), 0, 0, 300)
    har.backward(gy.cuda())
    Wr, br = W.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ref = orc.sine_source(f0, {"m.l_linear.weight": Wr, "m.l_linear.bias": br}, "m", 300, noise)[..., 0]
    ref.backward(gy)
    assert _rel(har.detach(), ref.detach()) < 1e-5
    assert _rel(Wd.grad, Wr.grad) < 1e-4 and _rel(bd.grad, br.grad) < 1e-4


def test_time_expand():
    from stts2_mi355x import training as T
    torch.manual_seed(1)
    y = torch.randn(2, 9, 13, 5, dtype=torch.float64)
    g = torch.randn(2, 9, 13, 15, dtype=torch.float64)
    yd = y.float().cuda().requires_grad_(True)
    x3 = T._TimeExpandFn.apply(yd)
    x3.backward(g.float().cuda())
    yr = y.clone().requires_grad_(True)
    pad = torch.nn.functional.pad(yr, (0, 0, 0, 0, 1, 1))
    ref = torch.stack([pad[:, dh:dh + 9] for dh in range(3)], dim=-1).reshape(2, 9, 13, 15)
    ref.backward(g)
    assert _rel(x3.detach(), ref.detach()) < 1e-7 and _rel(yd.grad, yr.grad) < 1e-6


@pytest.mark.parametrize("res", orc.MSD_RES)
@pytest.mark.parametrize("L", [4800, 4801])
def test_stft_mag_grads(res, L):
    from stts2_mi355x import training as T
    n_fft, hop, win = res
    torch.manual_seed(L)
    x = torch.randn(3, L, dtype=torch.float64)
    xd = x.float().cuda().requires_grad_(True)
    mag = T.stft_mag(xd, n_fft, hop, win)
    g = torch.randn(mag.shape, dtype=torch.float64)
    mag.backward(g.float().cuda())
    xr = x.clone().requires_grad_(True)
    ref = torch.stft(xr, n_fft, hop, win, torch.hann_window(win, dtype=torch.float64), return_complex=True)
    ref = ref.abs().transpose(1, 2)
    ref.backward(g)
    assert _rel(mag.detach(), ref.detach()) < 1e-5
    assert _rel(xd.grad, xr.grad) < 1e-5


@pytest.mark.parametrize("scale", [0.01, 3.0])  # TPRLS active (L_rel < tau) / inactive
def test_gan_terms(scale):
    from stts2_mi355x import losses as Lo
    torch.manual_seed(int(scale * 100))
    # fp32, as the reference computes: the TPRLS mask `dr < dg + m` decides the median element itself by
    # the rounding of dg + m, so the checker must see the same fp32 values
    shapes = [(2, 37), (2, 101), (2, 640)]
    dr = [torch.randn(s) * scale for s in shapes]
    dg = [torch.randn(s) * scale for s in shapes]
    fr = [[torch.randn(2, 8, 11, 3), torch.randn(2, 1, 11, 3)]]
    fg = [[torch.randn(2, 8, 11, 3), torch.randn(2, 1, 11, 3)]]

    def both(fn_ours, fn_ref, *lists):
        flat = [t for lst in lists for t in (lst if isinstance(lst[0], torch.Tensor) else [u for v in lst for u in v])]
        dev = [t.float().cuda().requires_grad_(True) for t in flat]
        ref = [t.clone().requires_grad_(True) for t in flat]

        def rebuild(ts):
            out, i = [], 0
            for lst in lists:
                if isinstance(lst[0], torch.Tensor):
                    out.append(ts[i:i + len(lst)])
                    i += len(lst)
                else:
                    grp = []
                    for v in lst:
                        grp.append(ts[i:i + len(v)])
                        i += len(v)
                    out.append(grp)
            return out
        lo = fn_ours(*rebuild(dev))
        lr = fn_ref(*rebuild(ref))
        lo.backward()
        lr.backward()
        assert abs(float(lo.detach()) - float(lr.detach())) <= 1e-5 * max(1.0, abs(float(lr.detach())))
        for a, b in zip(dev, ref):
            assert _rel(a.grad, b.grad, floor=1e-12) < 1e-5
        return float(lr)

    both(lambda r, g: Lo.discriminator_loss(r, g)[0], orc.discriminator_loss, dr, dg)
    both(lambda g: Lo.generator_loss(g)[0], orc.generator_loss, dg)
    both(Lo.feature_loss, orc.feature_loss, fr, fg)
    v1 = both(Lo.discriminator_TPRLS_loss, orc.discriminator_tprls_loss, dr, dg)
    v2 = both(Lo.generator_TPRLS_loss, orc.generator_tprls_loss, dr, dg)
    if scale < 1:
        assert v1 < 3 * orc.TAU and v2 < 3 * orc.TAU  # the relu is active: the gradients are not zero


def test_mrstft_loss_grad():
    from stts2_mi355x.losses import MultiResolutionSTFTLoss
    x = _waves(2, 4800, 3)[:, 0] * 0.7
    y = _waves(2, 4800, 4)[:, 0]
    xd = x.cuda().requires_grad_(True)
    loss = MultiResolutionSTFTLoss()(xd, y.cuda())
    loss.backward()
    xr = x.clone().requires_grad_(True)
    lr = orc.mrstft_loss(xr, y)
    lr.backward()
    assert abs(float(loss) - float(lr)) < 1e-5 * abs(float(lr))
    print("mrstft grad rel err", _rel(xd.grad, xr.grad))
    assert _rel(xd.grad, xr.grad) < 1e-3


def test_adamw_matches_torch():
    from stts2_mi355x.optim import AdamW
    torch.manual_seed(5)
    shapes = [(1000,), (33, 7), (1,), (4097,)]
    ps = [torch.randn(s) for s in shapes]
    pd = [p.clone().cuda().requires_grad_(True) for p in ps]
    pc = [p.clone().requires_grad_(True) for p in ps]
    od = AdamW(pd, lr=1e-4, betas=(0.0, 0.99), eps=1e-9, weight_decay=1e-4)
    oc = torch.optim.AdamW(pc, lr=1e-4, betas=(0.0, 0.99), eps=1e-9, weight_decay=1e-4, foreach=False)
    for it in range(3):
        gs = [torch.randn(s) * 10 ** (-it) for s in shapes]
        for a, b, g in zip(pd, pc, gs):
            a.grad, b.grad = g.cuda(), g.clone()
        od.step()
        oc.step()
    for a, b in zip(pd, pc):
        # the scalars come in as doubles and are formed as torch forms them: every element within one fp32 ulp of
        # torch's (its vectorised CPU loops may contract a product and a sum into one FMA where we do not), the
        # spacing taken at |b| and floored at 1e-11 for elements near zero (where the ulp of the decayed parameter
        # the update is subtracted from, not of the result, is the rounding step)
        a, b = a.detach().cpu(), b.detach()
        ulp = torch.nextafter(b.abs(), torch.tensor(float("inf"))) - b.abs()
        assert ((a - b).abs() <= ulp.clamp_min(1e-11)).all(), (a - b).abs().max().item()
    sd = od.state_dict()
    assert sd["state"][0]["step"].item() == 3 and set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    # a reloaded optimizer continues from the saved step counts (new step tensors, new host views of them)
    pd2 = [p.detach().clone().requires_grad_(True) for p in pd]
    od2 = AdamW(pd2, lr=1e-4, betas=(0.0, 0.99), eps=1e-9, weight_decay=1e-4)
    od2.load_state_dict(copy.deepcopy(sd))  # (torch shares same-device state tensors with the source otherwise)
    g = [torch.randn(s).cuda() for s in shapes]
    for a, b, gg in zip(pd, pd2, g):
        a.grad, b.grad = gg.clone(), gg.clone()
    od.step()
    od2.step()
    assert all(torch.equal(a, b) for a, b in zip(pd, pd2))
    assert od.state_dict()["state"][0]["step"].item() == 4 == od2.state_dict()["state"][0]["step"].item()


# ------------------------------------------------------------------ whole modules vs the oracle's autograd
def test_decoder_grads_vs_oracle():
    """Every decoder parameter gradient and the input gradients (asr, F0_curve, N, s) of a fixed linear
    probe of the output, vs autograd through the oracle in fp64 (next to its fp32 run = the reference)."""
    B, T = 2, 8
    dec, _ = make_decoder("hifigan")
    sd = _sd(dec)
    asr, f0, n, s, _, noise = _train_inputs(B, T)
    r = torch.from_numpy(synth.normal("dec_probe", (B, 1, 600 * T))).float()
    dec = dec.cuda().eval()
    ins = [t.cuda().requires_grad_(True) for t in (asr, f0, n, s)]
    y = dec(*ins, noise=noise.cuda())
    (y * r.cuda()).sum().backward()
    refs = {}
    for dt in (torch.float32, torch.float64):
        leaf = {k: v.detach().to(dt).clone().requires_grad_(True) for k, v in sd.items()}
        ir = [t.detach().to(dt).clone().requires_grad_(True) for t in (asr, f0, n, s)]
        yr = orc.decoder_hifigan(*ir, leaf, HIFI_CFG, noise)
        (yr * r.to(dt)).sum().backward()
        refs[dt] = (yr.detach(), {k: v.grad for k, v in leaf.items()}, {i: t.grad for i, t in enumerate(ir)})
    assert _rel(y.detach(), refs[torch.float64][0]) < 1e-4
    _check3({k: p.grad for k, p in dec.named_parameters()}, refs[torch.float32][1], refs[torch.float64][1],
            "decoder params")
    _check3({i: t.grad for i, t in enumerate(ins)}, refs[torch.float32][2], refs[torch.float64][2], "decoder inputs")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_decoder_concurrent_branches_match_serial(dtype):
    """training.CONCURRENT_BRANCHES (the generator's noise branch beside snake -> ups, and a stage's three
    resblocks, each on its own HIP stream) against one stream: output, every parameter gradient and the four
    input gradients bit-identical (the same launches, only their overlap differs)."""
    from stts2_mi355x import training as TR
    B, T = 2, 40
    dec, _ = make_decoder("hifigan")
    dec = dec.cuda().eval()
    asr, f0, n, s, _, noise = _train_inputs(B, T)
    r = torch.from_numpy(synth.normal("dec_probe_conc", (B, 1, 600 * T))).float().cuda()
    out = {}
    try:
        for conc in (False, True):
            TR.CONCURRENT_BRANCHES = conc
            dec.zero_grad(set_to_none=True)
            ins = [t.cuda().requires_grad_(True) for t in (asr, f0, n, s)]
            y = dec(*ins, noise=noise.cuda(), dtype=dtype)
            (y * r).sum().backward()
            torch.cuda.synchronize()
            out[conc] = (y.detach().clone(), {k: p.grad.clone() for k, p in dec.named_parameters()},
                         [t.grad.clone() for t in ins])
    finally:
        TR.CONCURRENT_BRANCHES = True
    a, b = out[False], out[True]
    assert torch.equal(a[0], b[0])
    assert all(torch.equal(a[1][k], b[1][k]) for k in a[1])
    assert all(torch.equal(u, v) for u, v in zip(a[2], b[2]))


def test_decoder_train_mode_smoothing():
    """.train() applies hifigan.py:447-455 with Python's random: replay the same draws into the oracle."""
    B, T = 1, 8
    dec, _ = make_decoder("hifigan")
    sd = _sd(dec)
    asr, f0, n, s, _, noise = _train_inputs(B, T)
    dec = dec.cuda().train()
    for seed in (1, 2, 3):
        random.seed(seed)
        with torch.no_grad():
            y = dec(asr.cuda(), f0.cuda(), n.cuda(), s.cuda(), noise=noise.cuda())
        random.seed(seed)
        smooth = ([0, 3, 7][random.randint(0, 2)], [0, 3, 7, 15][random.randint(0, 3)])
        ref = orc.decoder_hifigan(asr, f0, n, s, sd, HIFI_CFG, noise, smooth=smooth)
        print("smoothing", smooth, _rel(y, ref))
        assert _rel(y.cpu(), ref) < 1e-4
    # with autograd: the smoothing sits in the graph (d F0_curve passes through the box filter)
    random.seed(7)
    f0d = f0.cuda().requires_grad_(True)
    y = dec(asr.cuda(), f0d, n.cuda(), s.cuda(), noise=noise.cuda())
    y.sum().backward()
    random.seed(7)
    smooth = ([0, 3, 7][random.randint(0, 2)], [0, 3, 7, 15][random.randint(0, 3)])
    f0r = f0.clone().requires_grad_(True)
    orc.decoder_hifigan(asr, f0r, n, s, sd, HIFI_CFG, noise, smooth=smooth).sum().backward()
    assert _rel(f0d.grad, f0r.grad) < 1e-4


def test_discriminator_grads_vs_oracle():
    from stts2_mi355x.losses import DiscriminatorLoss
    mpd, msd = _discs()
    psd, ssd = _sd(mpd), _sd(msd)
    y = _waves(2, 4801, 0)
    yh = _waves(2, 4801, 1)
    mpd, msd = mpd.cuda(), msd.cuda()
    loss = DiscriminatorLoss(mpd, msd)(y.cuda(), yh.cuda())
    loss.backward()
    lp = {k: v.clone().requires_grad_(True) for k, v in psd.items()}
    ls = {k: v.clone().requires_grad_(True) for k, v in ssd.items()}
    lr = orc.discriminator_loss_all(y, yh, lp, ls)
    lr.backward()
    assert abs(float(loss) - float(lr)) < 1e-4 * abs(float(lr))
    _check_grads({k: p.grad for k, p in mpd.named_parameters()}, {k: v.grad for k, v in lp.items()}, what="mpd")
    _check_grads({k: p.grad for k, p in msd.named_parameters()}, {k: v.grad for k, v in ls.items()}, what="msd")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_discriminators_concurrent_streams_match_serial(dtype):
    """discriminators.CONCURRENT (each period / resolution on its own HIP stream, autograd backward on the same
    streams) against the serial loop: the D-step loss with its parameter gradients and the G-step loss with its
    input gradient, bit-identical (the same launches, only their overlap differs)."""
    from stts2_mi355x import discriminators as D
    from stts2_mi355x.losses import DiscriminatorLoss, GeneratorLoss
    mpd, msd = (m.cuda() for m in _discs())
    mpd.dtype_compute = msd.dtype_compute = dtype
    y = _waves(2, 4800, 0).cuda()
    yh = _waves(2, 4800, 1).cuda()
    out = {}
    try:
        for conc in (False, True):
            D.CONCURRENT = conc
            for p in list(mpd.parameters()) + list(msd.parameters()):
                p.grad = None
                p.requires_grad_(True)
            ld = DiscriminatorLoss(mpd, msd)(y, yh)
            ld.backward()
            gd = {k: p.grad.clone() for k, p in list(mpd.named_parameters()) + list(msd.named_parameters())}
            for p in list(mpd.parameters()) + list(msd.parameters()):
                p.requires_grad_(False)
            yhd = yh.clone().requires_grad_(True)
            lg = GeneratorLoss(mpd, msd)(y, yhd)
            lg.backward()
            torch.cuda.synchronize()
            out[conc] = (float(ld), gd, float(lg), yhd.grad.clone())
    finally:
        D.CONCURRENT = True
        for p in list(mpd.parameters()) + list(msd.parameters()):
            p.requires_grad_(True)
    a, b = out[False], out[True]
    assert a[0] == b[0] and a[2] == b[2]
    assert all(torch.equal(a[1][k], b[1][k]) for k in a[1])
    assert torch.equal(a[3], b[3])


def test_generator_loss_input_grad_vs_oracle():
    """GeneratorLoss w.r.t. y_hat through both discriminators (the G step's path into the decoder), vs the
    oracle in fp64 next to its fp32 run (the |STFT| adjoint is ill-conditioned at near-zero bins: dX = g X / |X|)."""
    from stts2_mi355x.losses import GeneratorLoss
    mpd, msd = _discs()
    psd, ssd = _sd(mpd), _sd(msd)
    y = _waves(2, 4800, 0)
    yh = _waves(2, 4800, 1)
    mpd, msd = mpd.cuda().requires_grad_(False), msd.cuda().requires_grad_(False)
    yhd = yh.cuda().requires_grad_(True)
    loss = GeneratorLoss(mpd, msd)(y.cuda(), yhd)
    loss.backward()
    grads, vals = {}, {}
    for dt in (torch.float32, torch.float64):
        yhr = yh.detach().to(dt).clone().requires_grad_(True)
        lr = orc.generator_loss_all(y.to(dt), yhr, _sd64(psd) if dt == torch.float64 else psd,
                                    _sd64(ssd) if dt == torch.float64 else ssd)
        lr.backward()
        grads[dt], vals[dt] = yhr.grad, float(lr)
    assert abs(float(loss) - vals[torch.float64]) < 1e-4 * abs(vals[torch.float64])
    _check3({"y_hat": yhd.grad}, {"y_hat": grads[torch.float32]}, {"y_hat": grads[torch.float64]}, "d GeneratorLoss / d y_hat")


# ------------------------------------------------------------------ the assembled step
def _summary_check(ours, fx, tag, floor_frac=1e-3, tol=1e-4, norm_tol=None):
    """Per tensor: the values at the fixture's probe indices and the L2 norm, relative to the tensor's max
    |g| (floored at floor_frac of the module's).  norm_tol: also the error relative to the module's max |g|."""
    names = [str(k) for k in fx[f"{tag}.names"]]
    gmax = float(fx[f"{tag}.maxabs"].max())
    worst, worst_n = (0.0, ""), (0.0, "")
    for i, k in enumerate(names):
        g = ours[k].detach().double().cpu().reshape(-1)
        scale = max(float(fx[f"{tag}.maxabs"][i]), floor_frac * gmax)
        e_val = float((g[torch.from_numpy(fx[f"{tag}.idx"][i])] - torch.from_numpy(fx[f"{tag}.val"][i])).abs().max())
        e_l2 = abs(float(g.norm()) - float(fx[f"{tag}.l2"][i])) / max(float(fx[f"{tag}.l2"][i]), scale)
        worst = max(worst, (e_val / scale, k), (e_l2, k + " (l2)"))
        worst_n = max(worst_n, (e_val / gmax, k))
    print(f"{tag}: worst {worst[0]:.2e} at {worst[1]}, module-normwise {worst_n[0]:.2e} ({len(names)} tensors)")
    assert worst[0] < tol, worst
    if norm_tol is not None:
        assert worst_n[0] < norm_tol, worst_n


def test_d_step_on_reference_output():
    """The D step alone on the reference's own y_rec (the fixture's): DiscriminatorLoss (losses.py:170-190)
    backward through the MPD and MSD, vs the oracle's fp64 autograd next to its fp32 run (the reference's
    computation: bit for bit on the survey container's CPU, tests/test_train_oracle_cpu.py; another CPU's
    BLAS rounds differently)."""
    from stts2_mi355x.losses import DiscriminatorLoss
    fx = golden("train_step_B2_T8")
    B, T = int(fx["B"]), int(fx["T"])
    mpd, msd = _discs()
    psd, ssd = _sd(mpd), _sd(msd)
    mpd, msd = mpd.cuda().train(), msd.cuda().train()
    wav = _train_inputs(B, T)[4]
    y_rec = torch.from_numpy(fx["y_rec"])
    d_loss = DiscriminatorLoss(mpd, msd)(wav.cuda(), y_rec.cuda()).mean()
    d_loss.backward()
    assert abs(float(d_loss) - float(fx["d_loss"])) <= 1e-5 * float(fx["d_loss"])
    refs = {}
    for dt in (torch.float32, torch.float64):
        lp = {k: v.detach().to(dt).clone().requires_grad_(True) for k, v in psd.items()}
        ls = {k: v.detach().to(dt).clone().requires_grad_(True) for k, v in ssd.items()}
        orc.discriminator_loss_all(wav.to(dt), y_rec.to(dt), lp, ls).backward()
        refs[dt] = ({k: v.grad for k, v in lp.items()}, {k: v.grad for k, v in ls.items()})
    # the discriminators' LeakyReLU(0.1): a pre-activation within fp32 rounding of 0 takes the other branch in
    # one implementation (tools/diag_mpd_grad.py: ours 1 sign flip vs fp64 in period 5's fmap3 here, the
    # reference 0), moving the flipped layer's own bias / weight gradients by up to 1.5e-3 of their max |g|
    # (profiles/r03_diag_mpd_kink.txt: convs.3.bias 1.17e-3, convs.3.weight_v 1.54e-3) and the layers below
    # by ~3e-4: per tensor 2e-3, and 1e-4 of the module's max |g|
    _check3({k: p.grad for k, p in mpd.named_parameters()}, refs[torch.float32][0], refs[torch.float64][0], "D step mpd",
            abs_tol=2e-3, norm_tol=1e-4)
    _check3({k: p.grad for k, p in msd.named_parameters()}, refs[torch.float32][1], refs[torch.float64][1], "D step msd",
            abs_tol=1e-3, norm_tol=1e-4)


def test_train_step_vs_reference_fixture():
    """One D + G step with AdamW (train.py:267-327) against the reference's own autograd and torch AdamW."""
    from stts2_mi355x.trainstep import TrainStep
    fx = golden("train_step_B2_T8")
    B, T = int(fx["B"]), int(fx["T"])
    dec, _ = make_decoder("hifigan")
    mpd, msd = _discs()
    p0 = {k: v.detach().clone() for k, v in dec.state_dict().items()}
    m0 = {k: v.detach().clone() for k, v in mpd.state_dict().items()}
    dec, mpd, msd = dec.cuda().eval(), mpd.cuda().train(), msd.cuda().train()
    asr, f0, n, s, wav, noise = _train_inputs(B, T)
    ins = [t.cuda().requires_grad_(True) for t in (asr, f0, n, s)]
    step = TrainStep(dec, mpd, msd, capture=True)
    out = step(*ins, wav.cuda(), noise=noise.cuda())
    torch.cuda.synchronize()
    assert _rel(out["y_rec"], fx["y_rec"]) < 1e-4
    for k in ("d_loss", "loss_mel", "loss_gen_all", "g_loss"):
        assert abs(float(out[k]) - float(fx[k])) <= 1e-4 * abs(float(fx[k])), (k, float(out[k]), float(fx[k]))
    # end to end (our y_rec differs from the reference's by fp32 rounding, ~1e-6, which reaches every
    # gradient through ~50 layers, the TPRLS medians and the AdamW-updated discriminators; the reference's
    # own fp32 gradients are 1.6e-4 - 3.3e-4 of max |g| from fp64 here): 1e-3 per tensor, 1e-4 module-normwise
    _summary_check(step.captured["mpd"], fx, "grad.mpd", tol=1e-3, norm_tol=1e-4)
    _summary_check(step.captured["msd"], fx, "grad.msd", tol=1e-3, norm_tol=1e-4)
    _summary_check(step.captured["dec"], fx, "grad.dec", tol=1e-3, norm_tol=1e-4)
    for i, k in enumerate(("asr", "F0_curve", "N", "s")):
        e = _rel(ins[i].grad, fx["grad_in." + k])
        print("input grad", k, e)
        assert e < 1e-3
    # the AdamW updates (first step: ~ -lr sign(g) - lr wd p) where the gradient is well above rounding
    # (tolerance: 2 fp32 ulps of the parameter; the update itself is ~ lr = 1e-5 / 1e-4)
    names = [str(k) for k in fx["grad.dec.names"]]
    sd1 = dec.state_dict()
    for i, k in enumerate(names):
        ix = torch.from_numpy(fx["grad.dec.idx"][i])
        old = p0[k].double().reshape(-1)[ix]
        d = sd1[k].cpu().double().reshape(-1)[ix] - old
        # entries whose gradient is well above its rounding level (a conv bias feeding an InstanceNorm has a
        # true gradient of 0: its sign, and so its update, is noise in any fp32 implementation)
        gm = float(fx["grad.dec.maxabs"].max())
        sig = np.abs(fx["grad.dec.val"][i]) > 1e-2 * max(float(fx["grad.dec.maxabs"][i]), 1e-3 * gm)
        tol = 2.4e-7 * np.abs(old.numpy()) + 1e-12
        assert (np.abs(d.numpy() - fx["grad.dec.delta"][i]) <= tol)[sig].all(), k
    md = mpd.state_dict()
    for i, k in enumerate(sorted(m0)):
        ix = torch.from_numpy(np.minimum((synth.hash_u01("probe_idx." + k, 24) * m0[k].numel()).astype(np.int64),
                                         m0[k].numel() - 1))
        old = m0[k].double().reshape(-1)[ix]
        d = md[k].cpu().double().reshape(-1)[ix] - old
        tol = 2.4e-7 * np.abs(old.numpy()) + 1e-12
        ok = np.abs(d.numpy() - fx["mpd.delta"][i]) <= tol
        assert ok.mean() >= 0.9, k  # entries whose gradient sits at rounding level may take the other sign


def test_train_step_config5_shape():
    """The config-5 shape (B = 2 segments of 155 frames = 93,000 samples, train.py:235 max_len 310) vs the
    oracle's step on the CPU."""
    from stts2_mi355x.trainstep import TrainStep
    B, T = 2, 155
    dec, _ = make_decoder("hifigan")
    mpd, msd = _discs()
    sds = (_sd(dec), _sd(mpd), _sd(msd))
    asr, f0, n, s, wav, noise = _train_inputs(B, T)
    dec, mpd, msd = dec.cuda().eval(), mpd.cuda().train(), msd.cuda().train()
    ins = [t.cuda().requires_grad_(True) for t in (asr, f0, n, s)]
    step = TrainStep(dec, mpd, msd, capture=True)
    out = step(*ins, wav.cuda(), noise=noise.cuda())
    torch.cuda.synchronize()
    y_o, l_o, g_o, _ = orc.train_step(*sds, HIFI_CFG, asr, f0, n, s, wav, noise)
    assert _rel(out["y_rec"].cpu(), y_o) < 1e-4
    for k in ("d_loss", "loss_mel", "loss_gen_all"):
        print(k, float(out[k]), l_o[k])
        assert abs(float(out[k]) - l_o[k]) <= 1e-3 * abs(l_o[k]), k
    # module-normwise (each error relative to the module's largest |g|): at 93,000 samples the 186,000-term
    # sums of e.g. l_linear's gradient cancel to ~1e-3 of their terms, so per-tensor relative errors of any
    # fp32 implementation (the oracle's included) are large there
    # (the decoder's gradients at this size are pinned against fp64 by test_decoder_grads_config5_shape;
    # here the fp32 oracle is the yardstick, and its own error at 93,000 samples reaches ~1e-3 normwise)
    for tag, tol in (("mpd", 1e-4), ("msd", 1e-4), ("dec", 1e-3)):
        _check_grads(step.captured[tag], g_o[tag], tol=tol, what=f"config5 {tag} (normwise)", floor_frac=1.0)


def test_decoder_grads_config5_shape():
    """Decoder gradients of a fixed linear probe at the config-5 shape vs the fp64 truth and the fp32
    reference's own values (tests/golden/train_c5_decoder_grads.npz, tests/golden/make_golden_train_c5.py)."""
    fx = golden("train_c5_decoder_grads")
    B, T = int(fx["B"]), int(fx["T"])
    dec, _ = make_decoder("hifigan")
    asr, f0, n, s, _, noise = _train_inputs(B, T)
    r = torch.from_numpy(synth.normal("dec_probe_c5", (B, 1, 600 * T))).float()
    dec = dec.cuda().eval()
    ins = [t.cuda().requires_grad_(True) for t in (asr, f0, n, s)]
    y = dec(*ins, noise=noise.cuda())
    (y * r.cuda()).sum().backward()
    grads = dict(dec.named_parameters())
    names = [str(k) for k in fx["names"]]
    gm = float(fx["f64.maxabs"].max())
    worst, worst_ref = (0.0, ""), (0.0, "")
    for i, k in enumerate(names):
        g = grads[k].grad.detach().double().cpu().reshape(-1)[torch.from_numpy(fx["idx"][i])].numpy()
        scale = max(float(fx["f64.maxabs"][i]), 1e-3 * gm)
        eo = np.abs(g - fx["f64.val"][i]).max() / scale
        er = np.abs(fx["f32.val"][i] - fx["f64.val"][i]).max() / scale
        worst, worst_ref = max(worst, (eo, k)), max(worst_ref, (er, k))
        assert eo <= max(2.0 * er, 1e-4), (k, eo, er)
    print(f"config5 decoder probe: vs fp64 ours worst {worst[0]:.2e} ({worst[1]}), fp32 reference worst "
          f"{worst_ref[0]:.2e} ({worst_ref[1]})")
    for i, k in enumerate(("asr", "F0_curve", "N", "s")):
        eo = _rel(ins[i].grad, fx[f"f64.grad_in.{k}"])
        er = _rel(fx[f"f32.grad_in.{k}"], fx[f"f64.grad_in.{k}"])
        print(f"  input {k}: ours {eo:.2e}, fp32 reference {er:.2e}")
        assert eo <= max(2.0 * er, 1e-4), k


# ------------------------------------------------------------------ the bf16 step (the mode config 5 is timed in)
def _metrics(ours, ref):
    """Module-level agreement of a gradient dict with the truth: the worst error relative to the module's
    largest |g| (normwise), the cosine similarity of the whole module's gradient vector, and the smallest
    per-tensor cosine over tensors carrying >= 1e-3 of the module's largest gradient norm."""
    keys = [k for k, g in ref.items() if g is not None]
    gm = max(float(ref[k].abs().max()) for k in keys)
    nmax = max(float(ref[k].norm()) for k in keys)
    normwise, dot, no, nr, cmin = 0.0, 0.0, 0.0, 0.0, (1.0, "")
    for k in keys:
        o, r = ours[k].detach().double().cpu().reshape(-1), ref[k].detach().double().cpu().reshape(-1)
        normwise = max(normwise, float((o - r).abs().max()) / gm)
        dot, no, nr = dot + float(o @ r), no + float(o @ o), nr + float(r @ r)
        if float(r.norm()) >= 1e-3 * nmax:
            c = float(o @ r) / max(float(o.norm() * r.norm()), 1e-300)
            cmin = min(cmin, (c, k))
    return {"normwise": normwise, "cos": dot / max((no * nr) ** 0.5, 1e-300), "cos_min": cmin[0], "cos_min_at": cmin[1]}


def _update_sign_agreement(p0, p1, ref_p1, ref_g):
    """Fraction of entries whose AdamW update has the truth's sign, over entries whose true gradient is above
    1e-2 of its tensor's max |g| (first step, beta1 = 0: the update is ~ -lr sign(g))."""
    agree = total = 0
    for k, g in ref_g.items():
        if g is None:
            continue
        g = g.detach().double().cpu().reshape(-1)
        sig = g.abs() > 1e-2 * float(g.abs().max())
        d = (p1[k].detach().double().cpu().reshape(-1) - p0[k].double().reshape(-1))[sig]
        dr = (ref_p1[k].detach().double().cpu().reshape(-1) - p0[k].double().reshape(-1))[sig]
        agree += int((torch.sign(d) == torch.sign(dr)).sum())
        total += int(sig.sum())
    return agree / max(total, 1)


def _run_step(dtype, B, T, sds=None):
    from stts2_mi355x.trainstep import TrainStep
    dec, _ = make_decoder("hifigan")
    mpd, msd = _discs()
    if sds is not None:
        for m, sd in zip((dec, mpd, msd), sds):
            m.load_state_dict(sd)
    p0 = tuple(_sd(m) for m in (dec, mpd, msd))
    asr, f0, n, s, wav, noise = _train_inputs(B, T)
    dec, mpd, msd = dec.cuda().eval(), mpd.cuda().train(), msd.cuda().train()
    ins = [t.cuda().requires_grad_(True) for t in (asr, f0, n, s)]
    step = TrainStep(dec, mpd, msd, dtype=dtype, capture=True)
    out = step(*ins, wav.cuda(), noise=noise.cuda())
    torch.cuda.synchronize()
    p1 = {"dec": _sd(dec), "mpd": _sd(mpd), "msd": _sd(msd)}
    assert mpd.dtype_compute == "fp32" and msd.dtype_compute == "fp32"  # the step's dtype does not leak
    return out, step.captured, p0, p1, {k: t.grad for k, t in zip(("asr", "F0_curve", "N", "s"), ins)}


# bounds of the bf16 step, about 2-3x the measured values (B2_T8 vs fp64 / config 5 vs the fp32
# step): module-normwise gradient error (dec 3.5e-4 / 7.8e-4, mpd 1.0e-4 / 5.8e-5, msd 5.0e-3 / 5.4e-3, input
# gradients 6.6e-2), whole-module cosine (>= 0.99986 for the parameters, 0.9986 for the inputs), smallest per-tensor
# cosine (>= 0.976 / 0.909: MSD's first weight_v), AdamW update sign agreement where |g| > 1e-2 max (>= 0.994 /
# 0.977), relative loss error (<= 2.7e-4)
BF16_STEP_BOUNDS = {"loss": 1e-3,
                    "normwise": {"dec": 2e-3, "mpd": 5e-4, "msd": 2e-2, "inputs": 0.2},
                    "cos": {"dec": 0.9999, "mpd": 0.9999, "msd": 0.9995, "inputs": 0.995},
                    "cos_min": {"dec": 0.95, "mpd": 0.995, "msd": 0.8, "inputs": 0.95},
                    "sign": {"dec": 0.97, "mpd": 0.995, "msd": 0.95}}


def _assert_bounds(tag, m):
    bd = BF16_STEP_BOUNDS
    assert m["normwise"] < bd["normwise"][tag], (tag, m)
    assert m["cos"] > bd["cos"][tag], (tag, m)
    assert m["cos_min"] > bd["cos_min"][tag], (tag, m)
    if "sign" in m:
        assert m["sign"] > bd["sign"][tag], (tag, m)


def test_train_step_bf16_vs_fp64():
    """TrainStep(dtype='bf16') at the fixture's size (B = 2 x 4,800 samples) against the oracle's step in fp64
    (the truth) next to our fp32 step: the four losses, every decoder / MPD / MSD gradient (module-normwise and
    by cosine), the input gradients and the sign of the AdamW updates."""
    B, T = 2, 8
    res = {dt: _run_step(dt, B, T) for dt in ("fp32", "bf16")}
    p0 = res["fp32"][2]
    d64 = lambda sd: {k: v.double() for k, v in sd.items()}  # noqa: E731
    asr, f0, n, s, wav, noise = (t.double() for t in _train_inputs(B, T))
    y64, l64, g64, par64 = orc.train_step(*(d64(sd) for sd in p0), HIFI_CFG, asr, f0, n, s, wav, noise)
    rows = {}
    for dt, (out, cap, _, p1, gin) in res.items():
        row = {"y_rec": _rel(out["y_rec"], y64)}
        for k in ("d_loss", "loss_mel", "loss_gen_all", "g_loss"):
            row[k] = abs(float(out[k]) - l64[k]) / abs(l64[k])
        for tag, i in (("dec", 0), ("mpd", 1), ("msd", 2)):
            row[tag] = _metrics(cap[tag], g64[tag])
            row[tag]["sign"] = _update_sign_agreement(p0[i], p1[tag], par64[tag], g64[tag])
        row["inputs"] = _metrics(gin, g64["inputs"])
        rows[dt] = row
        print(dt, {k: (v if not isinstance(v, dict) else {a: (round(b, 6) if isinstance(b, float) else b)
                                                           for a, b in v.items()}) for k, v in row.items()})
    r = rows["bf16"]
    for k in ("d_loss", "loss_mel", "loss_gen_all", "g_loss"):
        assert r[k] < BF16_STEP_BOUNDS["loss"], (k, r[k])
    for tag in ("dec", "mpd", "msd", "inputs"):
        _assert_bounds(tag, r[tag])
    # the fp32 step is the tight one (the fixture tests above bound it per tensor)
    for tag in ("dec", "mpd", "msd"):
        assert rows["fp32"][tag]["normwise"] < 1e-3 and rows["fp32"][tag]["cos"] > 0.999999, (tag, rows["fp32"][tag])


def test_train_step_bf16_config5_shape():
    """The bf16 step at the config-5 shape (B = 2 x 93,000 samples) against the fp32 step on the same weights
    and inputs (the fp32 step is pinned to the oracle at this shape by test_train_step_config5_shape)."""
    B, T = 2, 155
    res = {dt: _run_step(dt, B, T) for dt in ("fp32", "bf16")}
    o32, c32, p0, p32, gin32 = res["fp32"]
    o16, c16, _, p16, gin16 = res["bf16"]
    print("y_rec", _rel(o16["y_rec"], o32["y_rec"]))
    for k in ("d_loss", "loss_mel", "loss_gen_all", "g_loss"):
        e = abs(float(o16[k]) - float(o32[k])) / abs(float(o32[k]))
        print(k, float(o16[k]), float(o32[k]), e)
        assert e < BF16_STEP_BOUNDS["loss"], k
    for tag, i in (("dec", 0), ("mpd", 1), ("msd", 2)):
        m = _metrics(c16[tag], c32[tag])
        m["sign"] = _update_sign_agreement(p0[i], p16[tag], p32[tag], c32[tag])
        print(tag, m)
        _assert_bounds(tag, m)
    m = _metrics(gin16, gin32)
    print("inputs", m)
    _assert_bounds("inputs", m)


def test_engine_sees_adamw_update():
    """The HIP AdamW writes parameters through raw pointers; it bumps their version counters, so a no-grad
    forward after the step repacks: decoder and MPD outputs equal those of freshly built modules on the
    updated state dict."""
    from stts2_mi355x.discriminators import MultiPeriodDiscriminator
    from stts2_mi355x.optim import AdamW
    B, T = 1, 8
    dec, _ = make_decoder("hifigan")
    mpd, _ = _discs()
    dec, mpd = dec.cuda().eval(), mpd.cuda()
    asr, f0, n, s, wav, noise = (t.cuda() for t in _train_inputs(B, T))
    with torch.no_grad():
        y0 = dec(asr, f0, n, s, noise=noise)
        m0 = mpd(wav, wav)[0][0]
    for m in (dec, mpd):
        opt = AdamW(m.parameters(), lr=1e-2)
        for p in m.parameters():
            p.grad = torch.ones_like(p)
        opt.step()
    with torch.no_grad():
        y1 = dec(asr, f0, n, s, noise=noise)
        m1 = mpd(wav, wav)[0][0]
        dec2, _ = make_decoder("hifigan")
        dec2.load_state_dict(dec.state_dict())
        y2 = dec2.cuda().eval()(asr, f0, n, s, noise=noise)
        mpd2 = MultiPeriodDiscriminator()
        mpd2.load_state_dict(mpd.state_dict())
        m2 = mpd2.cuda()(wav, wav)[0][0]
    assert _rel(y1, y0) > 1e-3 and _rel(m1[0], m0[0]) > 1e-3  # the update moved the outputs
    assert _rel(y1, y2) < 1e-5, _rel(y1, y2)  # the fp32 decode's statistics: fp64 atomics
    assert torch.equal(m1[0], m2[0]), _rel(m1[0], m2[0])


def test_train_step_bf16x3_vs_fp64():
    """TrainStep(dtype='bf16x3') (fp32 frames, every conv forward / dx as split bf16 hi + lo operands on the
    bf16 MFMA, weight gradients in fp32) at the fixture's size against the oracle's step in fp64: it carries
    fp32-class accuracy (module-normwise gradient error <= 1e-3 like the fp32 step, losses 1e-4)."""
    B, T = 2, 8
    out, cap, p0, p1, gin = _run_step("bf16x3", B, T)
    d64 = lambda sd: {k: v.double() for k, v in sd.items()}  # noqa: E731
    asr, f0, n, s, wav, noise = (t.double() for t in _train_inputs(B, T))
    y64, l64, g64, par64 = orc.train_step(*(d64(sd) for sd in p0), HIFI_CFG, asr, f0, n, s, wav, noise)
    print("y_rec", _rel(out["y_rec"], y64))
    assert _rel(out["y_rec"], y64) < 1e-4
    for k in ("d_loss", "loss_mel", "loss_gen_all", "g_loss"):
        e = abs(float(out[k]) - l64[k]) / abs(l64[k])
        print(k, e)
        assert e < 1e-4, (k, e)
    for tag, i in (("dec", 0), ("mpd", 1), ("msd", 2)):
        m = _metrics(cap[tag], g64[tag])
        m["sign"] = _update_sign_agreement(p0[i], p1[tag], par64[tag], g64[tag])
        print(tag, m)
        assert m["normwise"] < 1e-3 and m["cos"] > 0.999999 and m["sign"] > 0.99, (tag, m)
    m = _metrics(gin, g64["inputs"])
    print("inputs", m)
    assert m["normwise"] < 1e-2 and m["cos"] > 0.9999, m


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_trainstep_graph_matches_eager(dtype):
    """TrainStep(graph=True): the config-5 step recorded in a hipGraph (device-side AdamW step counts, the noise seed
    read from the device) and replayed, against the eager step on twin modules over three steps with three seeds:
    the losses of every step and the parameters after the last within fp32 rounding of the AdamW scalars (the
    capturable form forms them in device fp64)."""
    from stts2_mi355x.trainstep import TrainStep
    B, T = 2, 16
    asr, f0, n, s, wav, _ = _train_inputs(B, T)
    mods = []
    for _ in range(2):
        dec, _ = make_decoder("hifigan")
        mpd, msd = _discs()
        mods.append((dec.cuda().eval(), mpd.cuda().train(), msd.cuda().train()))
    ins = [t.cuda().requires_grad_(True) for t in (asr, f0, n, s)]
    eager = TrainStep(*mods[0], dtype=dtype)
    graph = TrainStep(*mods[1], dtype=dtype, graph=True)
    for i in range(3):
        a = eager(*ins, wav.cuda(), seed=100 + i)
        b = graph(*ins, wav.cuda(), seed=100 + i)
        for k in ("d_loss", "loss_mel", "loss_gen_all", "g_loss"):
            ea, eb = float(a[k]), float(b[k])
            assert abs(ea - eb) <= 1e-6 * abs(ea) + 1e-7, (i, k, ea, eb)
        print(f"{dtype} step {i}: g_loss eager {float(a['g_loss']):.6f} graph {float(b['g_loss']):.6f}")
    assert graph._graph is not None
    worst = 0.0
    for (k, p), (_, q) in zip(mods[0][0].named_parameters(), mods[1][0].named_parameters()):
        d = float((p.detach() - q.detach()).abs().max())
        worst = max(worst, d / max(float(p.detach().abs().max()), 1e-6))
    print(f"{dtype}: decoder parameters after 3 steps, graph vs eager: worst rel {worst:.2e}")
    assert worst < 1e-5
    graph.opt["decoder"].sync_steps()
    st = graph.opt["decoder"].state[next(mods[1][0].parameters())]["step"]
    assert float(st) == 3.0


def test_capturable_adamw_checkpoint_roundtrip():
    """optim.AdamW(capturable=True) keeps the step count on the device: state_dict() folds it in (a checkpoint
    carries the real step, not the count at the first step), and load_state_dict() re-seeds the device count in
    place (a resumed optimizer's bias correction continues from the loaded step), also under TrainStep(graph=True),
    whose recorded graph keeps replaying with the re-seeded count.  Guards: a changed learning rate, another input
    shape and a train-mode decoder are refused by the graph path."""
    from stts2_mi355x.trainstep import TrainStep
    B, T = 2, 16
    asr, f0, n, s, wav, _ = _train_inputs(B, T)
    dec, _ = make_decoder("hifigan")
    mpd, msd = _discs()
    dec, mpd, msd = dec.cuda().eval(), mpd.cuda().train(), msd.cuda().train()
    ins = [t.cuda() for t in (asr, f0, n, s)]
    step = TrainStep(dec, mpd, msd, dtype="bf16", graph=True)
    for i in range(3):
        step(*ins, wav.cuda(), seed=10 + i)
    opt = step.opt["decoder"]
    sd = opt.state_dict()  # (no explicit sync_steps(): state_dict does it)
    steps = {float(v["step"]) for v in sd["state"].values()}
    assert steps == {3.0}, steps
    # resume: load a state saved at step 3 into an optimizer that has run 5 steps
    step(*ins, wav.cuda(), seed=20)
    step(*ins, wav.cuda(), seed=21)
    opt.load_state_dict(sd)
    dev = opt._dev_state[0]
    assert float(dev[0].item()) == 3.0
    step(*ins, wav.cuda(), seed=22)  # the recorded graph replays with the re-seeded count
    assert {float(v["step"]) for v in opt.state_dict()["state"].values()} == {4.0}
    # guards of the recorded step
    with pytest.raises(ValueError):
        step(ins[0][:, :, :8].contiguous(), ins[1][:, :16].contiguous(), ins[2][:, :16].contiguous(), ins[3],
             wav.cuda()[:, :, :4800].contiguous(), seed=1)
    opt.param_groups[0]["lr"] *= 2
    with pytest.raises(ValueError):
        step(*ins, wav.cuda(), seed=1)
    opt.param_groups[0]["lr"] /= 2
    dec.train()
    with pytest.raises(ValueError):
        step(*ins, wav.cuda(), seed=1)
    dec.eval()
    # the moments the recorded graph updates are the optimizer's state tensors after the load
    p0 = next(dec.parameters())
    before = opt.state[p0]["exp_avg"].clone()
    step(*ins, wav.cuda(), seed=23)
    assert not torch.equal(before, opt.state[p0]["exp_avg"])
