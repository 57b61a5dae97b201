"""The trainable iSTFTNet decoder on the MI355X: the new HIP layers (CustomSTFT transform, reflection-pad add,
exp / sin -> inverse-STFT head), the whole decoder, its dispatch and one TrainStep, forward and backward, against
autograd through the oracle's restatement of the reference (oracle/stts_oracle.py, fp64 on the CPU), which
tests/test_istftnet_train_cpu.py pins to the reference module's own gradients.  Errors are max |error| over max
|reference| (_rel, as tests/test_gpu_vocos_train.py): 1e-4 for a layer; the whole decoder by the rule of
tests/test_gpu_train_step.py (_check3)."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import ISTFT_CFG, decoder_case, golden, make_decoder
from oracle import stts_oracle as orc
from stts2_mi355x import synth
from test_gpu_train_step import _check3
from test_istftnet_train_cpu import NO_GRAD, _sample_idx, oracle_leaves

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HD_TF = 64  # frames per workgroup of the head kernels (csrc/istftnet_train.hip)


def _rel(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).abs().max() / max(ref.abs().max().item(), 1e-30))


def _stft_buffers(n_fft, hop):
    """The CustomSTFT buffers of the drop-in module under the oracle's state-dict keys (float32, as a checkpoint)."""
    from stts2_mi355x.istftnet import CustomSTFT
    return {"generator.stft." + k: v for k, v in CustomSTFT(n_fft, hop, n_fft).state_dict().items()}


# ------------------------------------------------------------------ layers
@pytest.mark.parametrize("n_fft,hop,L,B", [(20, 5, 10, 1),     # shorter than one window: both replicate pads overlap
                                           (20, 5, 1200, 2),   # the T = 2 source
                                           (16, 4, 37, 3)])    # L no multiple of hop
def test_cstft(n_fft, hop, L, B):
    """Magnitude to 1e-4 of max |ref|.  The phase as |angle difference mod 2 pi| where the reference magnitude
    exceeds 1e-3 of its maximum (below it atan2 is ill-conditioned): an error e on (re, im) turns the angle by at
    most e / mag, so the same absolute bound e = 1e-4 max |ref| is asked of phase error x magnitude."""
    from stts2_mi355x.training import cstft
    nb = n_fft // 2 + 1
    g = torch.Generator().manual_seed(100 * n_fft + L + B)
    wave = torch.tanh(torch.randn(B, L, generator=g))
    sd = _stft_buffers(n_fft, hop)
    mag_r, ph_r = orc.stft_transform(wave.double(), {k: v.double() for k, v in sd.items()}, n_fft, hop)  # [B, nb, F]
    out = cstft(wave.cuda(), sd["generator.stft.weight_forward_real"].cuda(),
                sd["generator.stft.weight_forward_imag"].cuda(), n_fft, hop)
    nF = L // hop + 1
    assert out.shape == (B, nF, n_fft + 2) and not out.requires_grad
    out = out.cpu().double().transpose(1, 2)
    mag, ph = out[:, :nb], out[:, nb:]
    mmax = mag_r.abs().max().item()
    e_mag = float((mag - mag_r).abs().max() / mmax)
    d = torch.remainder(ph - ph_r + math.pi, 2 * math.pi) - math.pi
    keep = mag_r > 1e-3 * mmax
    e_ph = float((d.abs() * mag_r)[keep].max() / mmax)
    print((n_fft, hop, L, B), f"mag {e_mag:.1e} phase x mag {e_ph:.1e} (largest angle error "
          f"{float(d.abs()[keep].max()):.1e} rad over {int(keep.sum())} of {keep.numel()} bins)")
    assert e_mag <= 1e-4
    assert e_ph <= 1e-4


@pytest.mark.parametrize("B,L,C", [(1, 2, 128), (2, 240, 128), (3, 5, 7)])
def test_padl_add(B, L, C):
    """Forward and both gradients bitwise equal to F.pad(x, (1, 0), 'reflect') + src on the device."""
    from stts2_mi355x.training import padl_add
    g = torch.Generator().manual_seed(B * 1000 + L + C)
    x = torch.randn(B, L, C, generator=g).cuda()
    src = torch.randn(B, L + 1, C, generator=g).cuda()
    R = torch.randn(B, L + 1, C, generator=g).cuda()
    xr, sr = x.clone().requires_grad_(True), src.clone().requires_grad_(True)
    y_ref = (F.pad(xr.transpose(1, 2), (1, 0), "reflect") + sr.transpose(1, 2)).transpose(1, 2)
    (y_ref * R).sum().backward()
    xd, sdv = x.clone().requires_grad_(True), src.clone().requires_grad_(True)
    y = padl_add(xd, sdv)
    (y * R).sum().backward()
    assert y.shape == (B, L + 1, C)
    assert torch.equal(y, y_ref)
    assert torch.equal(xd.grad, xr.grad)
    assert torch.equal(sdv.grad, sr.grad)


@pytest.mark.parametrize("n_fft,hop,nF,B", [(20, 5, 2, 1),             # fewer frames than the overlap
                                            (20, 5, 241, 2),           # the T = 2 shape: tile boundaries with halo
                                            (20, 5, HD_TF + 1, 1),     # one forward tile, two backward tiles
                                            (20, 5, HD_TF + 2, 1),     # one sample hop past the forward tile
                                            (16, 4, 37, 3),
                                            (64, 64, 3, 1),            # no overlap
                                            (4, 1, 9, 1)])
def test_cistft_head(n_fft, hop, nF, B):
    """audio and dpost against autograd through exp / sin + oracle.stft_inverse in fp64, to 1e-4 of max |ref| (the
    layer bound of tests/test_gpu_vocos_train.py); a second run is bitwise equal."""
    from stts2_mi355x.training import cistft_head
    nb = n_fft // 2 + 1
    g = torch.Generator().manual_seed(1000 * n_fft + 10 * nF + B)
    post = 0.5 * torch.randn(B, nF, 2 * nb, generator=g)  # exp stays below e^2
    R = torch.randn(B, (nF - 1) * hop, generator=g)
    sd = _stft_buffers(n_fft, hop)
    pr = post.double().requires_grad_(True)
    x = pr.transpose(1, 2)
    y_ref = orc.stft_inverse(torch.exp(x[:, :nb]), torch.sin(x[:, nb:]), {k: v.double() for k, v in sd.items()},
                             n_fft, hop).reshape(B, -1)
    (y_ref * R.double()).sum().backward()
    br = sd["generator.stft.weight_backward_real"].cuda()
    bi = sd["generator.stft.weight_backward_imag"].cuda()
    runs = []
    for _ in range(2):
        pd = post.cuda().requires_grad_(True)
        y = cistft_head(pd, br, bi, n_fft, hop)
        (y * R.cuda()).sum().backward()
        runs.append((y.detach(), pd.grad))
    y, dp = runs[0]
    assert y.shape == (B, (nF - 1) * hop)
    e_y, e_d = _rel(y, y_ref), _rel(dp, pr.grad)
    print((n_fft, hop, nF, B), f"audio {e_y:.1e} dpost {e_d:.1e}")
    assert e_y <= 1e-4 and e_d <= 1e-4
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


# ------------------------------------------------------------------ the whole decoder
_REFS = {}
_IN = ("asr", "F0_curve", "N", "s")


def _probe(B, L):
    return torch.from_numpy(synth.normal("istftnet_train_probe", (B, 1, L))).float()


def _oracle_grads(T, B):
    """(y, parameter grads, input grads, loss) of the oracle in fp32 and fp64 on the CPU, m_source.l_linear frozen
    (test_istftnet_train_cpu.oracle_leaves says why): computed once per case."""
    key = (T, B)
    if key not in _REFS:
        r = _probe(B, 600 * T)
        out = {}
        for dt in (torch.float32, torch.float64):
            leaf, names = oracle_leaves(dt)
            *ins, noise = decoder_case(B, T)
            ir = [t.to(dt).clone().requires_grad_(True) for t in ins]
            yr = orc.decoder_istft(*ir, leaf, ISTFT_CFG, noise)
            loss = (yr * r.to(dt)).sum()
            loss.backward()
            out[dt] = (yr.detach(), {k: leaf[k].grad for k in names}, {i: t.grad for i, t in enumerate(ir)},
                       float(loss.detach()))
        _REFS[key] = out
    return _REFS[key]


def _run(T, B, dtype="fp32", probe=None):
    dec = make_decoder("istftnet")[0].cuda()
    *ins, noise = decoder_case(B, T)
    ins = [t.cuda().requires_grad_(True) for t in ins]
    y = dec(*ins, noise=noise.cuda(), dtype=dtype)
    loss = (y * (probe if probe is not None else _probe(B, 600 * T).cuda())).sum()
    loss.backward()
    torch.cuda.synchronize()
    return y.detach(), {k: p.grad for k, p in dec.named_parameters()}, {i: t.grad for i, t in enumerate(ins)}, \
        float(loss.detach())


@pytest.mark.parametrize("T,B", [(4, 2), (7, 1)])
def test_decoder_grads_vs_oracle(T, B):
    """Output within the larger of 1e-4 of max |ref| and twice the oracle's own fp32-vs-fp64 error (the exp head may
    amplify rounding; both figures are printed); every parameter and input gradient as close to fp64 as the
    oracle's own fp32 run (x 2 for another summation order, floor 1e-4), and within 1e-4 of the module's largest
    gradient; m_source.l_linear gets none.

    Measured on the MI355X: T = 7, B = 1: y 3.8e-6 (the oracle's fp32 2.9e-6), parameters worst 1.7e-5, inputs
    worst 4.8e-6; T = 4, B = 2: y 9.2e-6 (4.1e-6), parameters worst 6.4e-5 (5.1e-5), inputs worst 6.6e-5 (asr; the
    oracle's fp32 3.2e-5).  At T = 4 every AdaIN1d of the front-end normalises over 4 frames and amplifies the
    rounding of the convs around it about 30x in d asr (each op alone, fed fp64 inputs, is within 4e-6), which is
    why the fp32 path sums its front-end convs in 512-channel blocks (training.conv1d_chunked): with one
    3,270-term chain per output the same case measured asr 1.09e-4."""
    refs = _oracle_grads(T, B)
    y, gp, gi, _ = _run(T, B)
    assert y.shape == (B, 1, 600 * T)
    e = _rel(y, refs[torch.float64][0])
    e32 = _rel(refs[torch.float32][0], refs[torch.float64][0])
    print(f"istftnet train T {T} B {B}: y vs fp64 {e:.2e}, the oracle's fp32 vs fp64 {e32:.2e}")
    assert e <= max(1e-4, 2 * e32)
    for k in NO_GRAD:
        assert gp[k] is None and refs[torch.float64][1][k] is None, k
    _check3(gp, refs[torch.float32][1], refs[torch.float64][1], "istftnet params", norm_tol=1e-4)
    _check3(gi, refs[torch.float32][2], refs[torch.float64][2], "istftnet inputs", norm_tol=1e-4)


@pytest.mark.parametrize("T,B", [(4, 2), (7, 1)])
def test_decoder_grads_vs_reference_fixture(T, B):
    """The same run with the fixture's probe against the reference module's own fp64 gradients
    (tests/golden/istftnet_train_*.npz: the input gradients in full, 64 samples per parameter), by the rule of
    _check3 with the fixture as the truth and the oracle's fp32 run as the fp32 reference."""
    fx = golden(f"istftnet_train_T{T}_B{B}")
    R = torch.randn(tuple(fx["out_shape"]), generator=torch.Generator().manual_seed(int(fx["r_seed"])),
                    dtype=torch.float64)
    _, gp, gi, loss = _run(T, B, probe=R.float().cuda())
    assert sorted(str(k) for k in fx["none"]) == NO_GRAD
    # the oracle in fp32 with the fixture's probe: the reference's own precision at this case
    leaf, names = oracle_leaves(torch.float32)
    *ins, noise = decoder_case(B, T)
    ir = [t.clone().requires_grad_(True) for t in ins]
    (orc.decoder_istft(*ir, leaf, ISTFT_CFG, noise) * R.float()).sum().backward()

    def pick(g):
        return g.detach().reshape(-1).cpu()[torch.from_numpy(_sample_idx(g.numel()))]

    fnames = [str(k) for k in fx["names"]]
    r64 = {k: torch.from_numpy(fx["val"][i]) for i, k in enumerate(fnames)}
    # (the sampled values of a tensor are scaled by the tensor's true max |g|: _check3 floors at 1e-3 of the largest
    # value it sees, and the fixture's maxabs row restores the full-tensor scale for that)
    r64["__gmax__"] = torch.tensor([float(fx["maxabs"].max())], dtype=torch.float64)
    ours = {k: pick(gp[k]) for k in fnames}
    r32 = {k: pick(leaf[k].grad) for k in fnames}
    ours["__gmax__"] = r32["__gmax__"] = r64["__gmax__"]
    for k in NO_GRAD:
        assert gp[k] is None
    print(f"istftnet T {T} B {B}: loss {loss:.6f} fixture {float(fx['loss']):.6f}")
    _check3(ours, r32, r64, "istftnet params vs the reference fixture", norm_tol=1e-4)
    _check3(gi, {i: t.grad for i, t in enumerate(ir)},
            {i: torch.from_numpy(fx["grad_in." + k]) for i, k in enumerate(_IN)},
            "istftnet inputs vs the reference fixture", norm_tol=1e-4)


def _corr(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    return float((a @ b) / max(float(a.norm() * b.norm()), 1e-300))


def test_decoder_bf16_modes_follow_fp32():
    """bf16 and bf16x3 select the conv-engine mode of the convs: the output, the loss terms (y * R) and the input
    gradients correlate with the fp32 run above 0.99 at T = 16, B = 2 (the project's bound for HiFi-GAN and Vocos);
    the max-abs errors are measured figures (printed and written to profiles/istftnet_train_dtype_err.txt)."""
    T, B = 16, 2
    y32, gp32, gi32, l32 = _run(T, B, "fp32")
    probe = _probe(B, 600 * T).cuda()
    lines = [f"istftnet decoder autograd path, n_fft 20 hop 5 T {T} B {B}: max-abs error vs the fp32 run"]
    fails = []
    for dt in ("bf16", "bf16x3"):
        y, gp, gi, loss = _run(T, B, dt)
        cy = _corr(y, y32)
        cl = _corr(y * probe, y32 * probe)  # the loss is the sum of these terms
        ci = {k: _corr(gi[i], gi32[i]) for i, k in enumerate(_IN)}
        ei = {k: float((gi[i] - gi32[i]).abs().max()) for i, k in enumerate(_IN)}
        keys = [k for k in gp32 if gp32[k] is not None]
        gmax = max(float(gp32[k].abs().max()) for k in keys)
        ep = max(float((gp[k] - gp32[k]).abs().max()) for k in keys)
        line = (f"{dt}: loss {loss:.6f} (fp32 {l32:.6f}, rel {abs(loss - l32) / abs(l32):.2e}), y max-abs "
                f"{float((y - y32).abs().max()):.3e} corr {cy:.6f}, loss terms corr {cl:.6f}, input grads max-abs "
                + ", ".join(f"{k} {v:.3e} (corr {ci[k]:.5f})" for k, v in ei.items())
                + f", params worst max-abs {ep:.3e} (largest |g| {gmax:.3e})")
        print(line)
        lines.append(line)
        if not (cy > 0.99 and cl > 0.99):
            fails.append((dt, "y / loss terms", cy, cl))
        fails += [(dt, k, c) for k, c in ci.items() if not c > 0.99]
    try:
        with open(os.path.join(ROOT, "profiles", "istftnet_train_dtype_err.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    except OSError:
        pass  # a read-only checkout: the figures are in the test's output
    assert not fails, fails


def test_decoder_grads_deterministic():
    a = _run(4, 2)
    b = _run(4, 2)
    assert torch.equal(a[0], b[0])
    for k in a[1]:
        if k in NO_GRAD:
            assert a[1][k] is None and b[1][k] is None
            continue
        assert torch.equal(a[1][k], b[1][k]), k
    for i in a[2]:
        assert torch.equal(a[2][i], b[2][i]), i


def test_dispatch():
    dec = make_decoder("istftnet")[0].cuda()
    *x, noise = [t.cuda() for t in decoder_case(1, 4)]
    y = dec(*x, noise=noise)
    assert y.grad_fn is not None and y.shape == (1, 1, 2400)
    with torch.no_grad():
        a = dec(*x, noise=noise)
        b = dec.engine("fp32").forward(*x, noise=noise)
    assert a.grad_fn is None and torch.equal(a, b)
    # frozen parameters, an input requiring grad: still the autograd path
    dec.requires_grad_(False)
    s = x[3].clone().requires_grad_(True)
    assert dec(x[0], x[1], x[2], s, noise=noise).grad_fn is not None
    # .train() mode without grad: the smoothing, then the inference engine
    dec.train()
    with torch.no_grad():
        c = dec(*x, noise=noise)
    assert c.shape == (1, 1, 2400) and c.grad_fn is None and torch.isfinite(c).all()


def test_train_step_with_istftnet_decoder():
    """One eager TrainStep with an iSTFTNet decoder and the MPD / MSD at B = 2, T = 10 (6,000 samples): finite
    losses, every decoder parameter but m_source.l_linear moved, none NaN; graph=True is refused."""
    from helpers import fill_module
    from stts2_mi355x.discriminators import MultiPeriodDiscriminator, MultiResSpecDiscriminator
    from stts2_mi355x.trainstep import TrainStep
    B, T = 2, 10
    dec = make_decoder("istftnet")[0].cuda()
    mpd = fill_module(MultiPeriodDiscriminator(), "mpd.").cuda().train()
    msd = fill_module(MultiResSpecDiscriminator(), "msd.").cuda().train()
    p0 = {k: v.detach().clone() for k, v in dec.named_parameters()}
    ins = [torch.from_numpy(a).cuda() for a in synth.decoder_inputs(B, T, tag="train")]
    wav = torch.from_numpy(synth.waves(B, 600 * T, 7)).cuda()
    with pytest.raises(NotImplementedError):
        TrainStep(dec, mpd, msd, graph=True)
    out = TrainStep(dec, mpd, msd)(*ins, wav, seed=1)
    torch.cuda.synchronize()
    assert out["y_rec"].shape == (B, 1, 600 * T)
    for k in ("d_loss", "loss_mel", "loss_gen_all", "g_loss"):
        assert torch.isfinite(out[k]).all(), (k, out[k])
    for k, p in dec.named_parameters():
        assert torch.isfinite(p).all(), k
        if k in NO_GRAD:
            assert p.grad is None and torch.equal(p.detach(), p0[k]), k
        else:
            assert not torch.equal(p.detach(), p0[k]), k
