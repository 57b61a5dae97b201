"""The trainable Vocos decoder on the MI355X: the new HIP layer pairs (depthwise conv, GELU, layer-scale residual,
ISTFT head), a ConvNeXt block, the whole decoder, its dispatch and one TrainStep, forward and backward, against
autograd through the oracle's restatement of the reference (oracle/stts_oracle.py, fp64 on the CPU), which
tests/test_vocos_train_cpu.py pins to the reference module's own gradients.  Errors are max |error| over max
|reference| (_rel, as tests/test_gpu_train_layers.py): 1e-4 for a layer, 2e-4 for a block; the whole decoder by
the rule of tests/test_gpu_train_step.py (_check3)."""
import os

import pytest
import torch
import torch.nn.functional as F

from oracle import stts_oracle as orc
from stts2_mi355x import synth
from test_gpu_train_step import _check3
from test_vocos_cpu import make_vocos
from test_vocos_train_cpu import HEAD_CASES, head_inputs, head_masks

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).abs().max() / max(ref.abs().max().item(), 1e-30))


# ------------------------------------------------------------------ layers
@pytest.mark.parametrize("B,L,C,K", [(2, 5, 512, 7),     # L shorter than the kernel: both pads overlap
                                     (1, 77, 512, 7),    # L no multiple of the rows per thread
                                     (3, 300, 64, 7),    # C below one block
                                     (2, 45, 300, 3)])   # K = 3, C no multiple of the block
def test_dwconv(B, L, C, K):
    from stts2_mi355x.training import dwconv1d_frames
    g = torch.Generator().manual_seed(B * 1000 + L + C + K)
    x = torch.randn(B, L, C, generator=g)
    w = torch.randn(C, 1, K, generator=g) * 0.4
    b = torch.randn(C, generator=g) * 0.1
    R = torch.randn(B, L, C, generator=g)
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
    y_ref = F.conv1d(xr.transpose(1, 2), wr, br, 1, K // 2, 1, C).transpose(1, 2)
    (y_ref * R.double()).sum().backward()
    xd, wd, bd = (t.cuda().requires_grad_(True) for t in (x, w, b))
    y = dwconv1d_frames(xd, wd, bd)
    (y * R.cuda()).sum().backward()
    errs = {"y": _rel(y, y_ref), "dx": _rel(xd.grad, xr.grad), "dw": _rel(wd.grad, wr.grad),
            "db": _rel(bd.grad, br.grad)}
    print((B, L, C, K), {k: f"{v:.1e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v < 1e-4, (k, v)


@pytest.mark.parametrize("n", [1, 1537, 2 * 300 * 1536])
def test_gelu(n):
    from stts2_mi355x.training import gelu
    g = torch.Generator().manual_seed(n)
    x = torch.rand(n, generator=g) * 12 - 6  # spans [-6, 6]
    if n > 2:
        x[0], x[1] = -6.0, 6.0
    R = torch.randn(n, generator=g)
    xr = x.double().requires_grad_(True)
    y_ref = F.gelu(xr)
    (y_ref * R.double()).sum().backward()
    xd = x.cuda().requires_grad_(True)
    y = gelu(xd)
    (y * R.cuda()).sum().backward()
    errs = {"y": _rel(y, y_ref), "dx": _rel(xd.grad, xr.grad)}
    print(n, {k: f"{v:.1e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v < 1e-4, (k, v)


def test_layer_scale_residual():
    from stts2_mi355x.training import layer_scale_res
    B, L, C = 2, 77, 512
    g = torch.Generator().manual_seed(5)
    x, r, R = (torch.randn(B, L, C, generator=g) for _ in range(3))
    gamma = torch.randn(C, generator=g) * 0.3
    xr, rr, gr = (t.double().requires_grad_(True) for t in (x, r, gamma))
    y_ref = rr + gr * xr
    (y_ref * R.double()).sum().backward()
    xd, rd, gd = (t.cuda().requires_grad_(True) for t in (x, r, gamma))
    y = layer_scale_res(xd, rd, gd)
    (y * R.cuda()).sum().backward()
    errs = {"y": _rel(y, y_ref), "dx": _rel(xd.grad, xr.grad), "dr": _rel(rd.grad, rr.grad),
            "dgamma": _rel(gd.grad, gr.grad)}
    print({k: f"{v:.1e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v < 1e-4, (k, v)


@pytest.mark.parametrize("n_fft,hop,nF,B", HEAD_CASES)
def test_istft_head(n_fft, hop, nF, B):
    """y and dh against autograd through the oracle's exp / clip / cos / sin + vocos_istft in fp64.  The clipped
    bins' d h_mag is exactly 0; bins within 1e-4 (relative) of the clip threshold are left out of the d h_mag
    comparison only (fp32 and fp64 may decide them differently); the DC and Nyquist phase channels get the
    oracle's gradient."""
    from stts2_mi355x.training import istft_head
    nb = n_fft // 2 + 1
    h, R = head_inputs(n_fft, hop, nF, B)
    clipped, near = head_masks(h, n_fft)
    window = torch.hann_window(n_fft)
    hr = h.double().requires_grad_(True)
    x = hr.transpose(1, 2)
    mag, p = x.chunk(2, dim=1)
    mag = torch.clip(torch.exp(mag), max=1e2)
    y_ref = orc.vocos_istft(mag * (torch.cos(p) + 1j * torch.sin(p)), window.double(), n_fft, hop)
    y_ref = y_ref.reshape(B, -1)
    (y_ref * R.double()).sum().backward()
    hd = h.cuda().requires_grad_(True)
    y = istft_head(hd, window.cuda(), n_fft, hop)
    assert y.shape == (B, nF * hop)
    (y * R.cuda()).sum().backward()
    dh, dh_ref = hd.grad.cpu().double(), hr.grad
    scale = dh_ref.abs().max().item()
    keep = ~near
    e_mag = float(((dh[..., :nb] - dh_ref[..., :nb]).abs() * keep).max() / scale)
    e_ph = float((dh[..., nb:] - dh_ref[..., nb:]).abs().max() / scale)
    e_edge = float((dh[..., [nb, 2 * nb - 1]] - dh_ref[..., [nb, 2 * nb - 1]]).abs().max() / scale)
    print((n_fft, hop, nF, B), f"y {_rel(y, y_ref):.1e} dh_mag {e_mag:.1e} dh_phase {e_ph:.1e} edge phase {e_edge:.1e}",
          f"clipped {clipped.double().mean().item():.3f} near {int(near.sum())}")
    assert _rel(y, y_ref) < 1e-4
    assert e_mag < 1e-4 and e_ph < 1e-4 and e_edge < 1e-4
    sure = clipped & keep
    assert sure.any() and (dh[..., :nb][sure] == 0).all()
    assert (dh_ref[..., :nb][sure] == 0).all()


def _init_block(blk, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in blk.named_parameters():
            if n == "gamma":
                p.copy_(0.125 + 0.05 * torch.randn(p.shape, generator=g))
            elif n.endswith("bias"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
            elif n == "dwconv.weight":
                p.copy_(torch.randn(p.shape, generator=g) * 0.4)
            else:
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)


def test_convnext_block():
    """One ConvNeXtBlock (dim 512, intermediate 1536): output, dx, ds and every parameter gradient against autograd
    through oracle.convnext_block in fp64.  dwconv.bias feeds the AdaIN's InstanceNorm, which cancels a per-channel
    shift: its true gradient is 0 and it is checked against the module's largest gradient instead."""
    from stts2_mi355x.training import convnext_block_frames
    from stts2_mi355x.vocos import ConvNeXtBlock
    B, L, C, S = 2, 40, 512, 128
    blk = ConvNeXtBlock(C, 1536, 0.125, S)
    _init_block(blk, 3)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(B, C, L, generator=g)
    s = torch.randn(B, S, generator=g)
    R = torch.randn(B, C, L, generator=g)
    sd = {"b." + k: v.detach().double().requires_grad_(True) for k, v in blk.state_dict().items()}
    xr, sr = x.double().requires_grad_(True), s.double().requires_grad_(True)
    y_ref = orc.convnext_block(xr, sr, sd, "b")
    (y_ref * R.double()).sum().backward()
    blk.cuda()
    xd, sdv = x.cuda().requires_grad_(True), s.cuda().requires_grad_(True)
    y = convnext_block_frames(blk, xd.transpose(1, 2), sdv, "fp32").transpose(1, 2)
    (y * R.cuda()).sum().backward()
    errs = {"y": _rel(y, y_ref), "dx": _rel(xd.grad, xr.grad), "ds": _rel(sdv.grad, sr.grad)}
    scale = max(sd["b." + n].grad.abs().max().item() for n, _ in blk.named_parameters())
    for n, p in blk.named_parameters():
        if n == "dwconv.bias":
            assert p.grad.abs().max().item() < 1e-5 * scale, n
            continue
        errs[n] = _rel(p.grad, sd["b." + n].grad)
    worst = max(errs, key=errs.get)
    print("convnext block worst", worst, f"{errs[worst]:.2e}", {k: f"{v:.1e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v < 2e-4, (k, v)


# ------------------------------------------------------------------ the whole decoder
CFG = {1200: dict(num_layers=8, n_fft=1200, hop=300), 1024: dict(num_layers=8, n_fft=1024, hop=256)}
_REFS = {}


def _inputs(B, T):
    return [torch.from_numpy(a) for a in synth.decoder_inputs(B, T, tag="vocos")]


def _probe(B, L):
    return torch.from_numpy(synth.normal("vocos_train_probe", (B, 1, L))).float()


def _oracle_grads(n_fft, hop, T, B):
    """(y, parameter grads, input grads) of the oracle in fp32 and fp64 on the CPU: computed once per case."""
    key = (n_fft, hop, T, B)
    if key not in _REFS:
        sd = {k: v.detach().clone() for k, v in make_vocos(n_fft, hop).state_dict().items()}
        names = [k for k, _ in make_vocos(n_fft, hop).named_parameters()]
        r = _probe(B, 2 * T * hop)
        out = {}
        for dt in (torch.float32, torch.float64):
            leaf = {k: v.to(dt).clone() for k, v in sd.items()}
            for k in names:
                leaf[k].requires_grad_(True)
            ir = [t.to(dt).clone().requires_grad_(True) for t in _inputs(B, T)]
            yr = orc.decoder_vocos(*ir, leaf, CFG[n_fft])
            loss = (yr * r.to(dt)).sum()
            loss.backward()
            out[dt] = (yr.detach(), {k: leaf[k].grad for k in names}, {i: t.grad for i, t in enumerate(ir)},
                       float(loss.detach()))
        _REFS[key] = out
    return _REFS[key]


def _run(n_fft, hop, T, B, dtype="fp32"):
    dec = make_vocos(n_fft, hop).cuda()
    ins = [t.cuda().requires_grad_(True) for t in _inputs(B, T)]
    y = dec(*ins, dtype=dtype)
    loss = (y * _probe(B, 2 * T * hop).cuda()).sum()
    loss.backward()
    torch.cuda.synchronize()
    return y.detach(), {k: p.grad for k, p in dec.named_parameters()}, {i: t.grad for i, t in enumerate(ins)}, \
        float(loss.detach())


@pytest.mark.parametrize("n_fft,hop,T,B", [(1200, 300, 4, 2), (1024, 256, 7, 1)])
def test_decoder_grads_vs_oracle(n_fft, hop, T, B):
    """Output to 1e-4; every parameter and input gradient as close to fp64 as the oracle's own fp32 run (x 2 for
    another summation order, floor 1e-4), and within 1e-4 of the module's largest gradient."""
    refs = _oracle_grads(n_fft, hop, T, B)
    y, gp, gi, _ = _run(n_fft, hop, T, B)
    assert y.shape == (B, 1, 2 * T * hop)
    e = _rel(y, refs[torch.float64][0])
    print(f"vocos train n_fft {n_fft} T {T} B {B}: y vs fp64 {e:.2e}")
    assert e < 1e-4
    _check3(gp, refs[torch.float32][1], refs[torch.float64][1], f"vocos {n_fft} params", norm_tol=1e-4)
    _check3(gi, refs[torch.float32][2], refs[torch.float64][2], f"vocos {n_fft} inputs", norm_tol=1e-4)


def _corr(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    return float((a @ b) / max(float(a.norm() * b.norm()), 1e-300))


def test_decoder_bf16_modes_follow_fp32():
    """bf16 and bf16x3 select the conv-engine mode of the convs and GEMMs: the loss (a linear probe of the output:
    its terms y * R, and the output itself) and the input gradients correlate with the fp32 run above 0.99; the
    max-abs errors are measured figures (printed and written to profiles/vocos_train_dtype_err.txt).

    The case is T = 16 (16 front-end frames, 32 ConvNeXt frames), not the T = 4 of the fp32 tests: every AdaIN1d
    normalises a channel by the standard deviation of its L frames, and over L = 4 frames a nearly constant channel
    turns the bf16 rounding of the conv before it (2^-9 relative) into an O(1) change of the normalised value, so
    that case measures its own conditioning (measured there: bf16 output corr 0.99981, input-gradient corr asr
    0.98775, F0_curve 0.99736, N 0.99469, s 0.98287).  The project's other bf16 agreement checks also use 8 frames
    or more (tests/test_gpu_train_step.py T = 8, tests/test_gpu_vocos.py T = 400)."""
    n_fft, hop, T, B = 1200, 300, 16, 2
    y32, gp32, gi32, l32 = _run(n_fft, hop, T, B, "fp32")
    probe = _probe(B, 2 * T * hop).cuda()
    lines = [f"vocos decoder autograd path, n_fft {n_fft} hop {hop} T {T} B {B}: max-abs error vs the fp32 run"]
    for dt in ("bf16", "bf16x3"):
        y, gp, gi, loss = _run(n_fft, hop, T, B, dt)
        cy = _corr(y, y32)
        cl = _corr(y * probe, y32 * probe)  # the loss is the sum of these terms
        ci = {k: _corr(gi[i], gi32[i]) for i, k in enumerate(("asr", "F0_curve", "N", "s"))}
        ei = {k: float((gi[i] - gi32[i]).abs().max()) for i, k in enumerate(("asr", "F0_curve", "N", "s"))}
        gmax = max(float(g.abs().max()) for g in gp32.values())
        ep = max(float((gp[k] - gp32[k]).abs().max()) for k in gp32)
        line = (f"{dt}: loss {loss:.6f} (fp32 {l32:.6f}, rel {abs(loss - l32) / abs(l32):.2e}), y max-abs "
                f"{float((y - y32).abs().max()):.3e} corr {cy:.6f}, loss terms corr {cl:.6f}, input grads max-abs "
                + ", ".join(f"{k} {v:.3e} (corr {ci[k]:.5f})" for k, v in ei.items())
                + f", params worst max-abs {ep:.3e} (largest |g| {gmax:.3e})")
        print(line)
        lines.append(line)
        assert cy > 0.99 and cl > 0.99, (dt, cy, cl)
        for k, c in ci.items():
            assert c > 0.99, (dt, k, c)
    try:
        with open(os.path.join(ROOT, "profiles", "vocos_train_dtype_err.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    except OSError:
        pass  # a read-only checkout: the figures are in the test's output


def test_decoder_grads_deterministic():
    a = _run(1200, 300, 4, 2)
    b = _run(1200, 300, 4, 2)
    assert torch.equal(a[0], b[0])
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k
    for i in a[2]:
        assert torch.equal(a[2][i], b[2][i]), i


def test_dispatch():
    dec = make_vocos(1200, 300).cuda()
    x = [t.cuda() for t in _inputs(1, 4)]
    y = dec(*x)
    assert y.grad_fn is not None and y.shape == (1, 1, 2400)
    with torch.no_grad():
        a = dec(*x)
        b = dec.engine("fp32").forward(*x)
    assert a.grad_fn is None and torch.equal(a, b)
    # frozen parameters, an input requiring grad: still the autograd path
    dec.requires_grad_(False)
    s = x[3].clone().requires_grad_(True)
    assert dec(x[0], x[1], x[2], s).grad_fn is not None
    # the source keywords are accepted (TrainStep passes them to every decoder) and ignored
    with torch.no_grad():
        c = dec(*x, noise=None, seed=3, utt_offset=1)
    assert torch.equal(a, c)


def test_train_step_with_vocos_decoder():
    """One eager TrainStep with a Vocos decoder (n_fft 1200, hop 300) and the MPD / MSD at B = 2, T = 10 (6,000
    samples): finite losses, every decoder parameter moved, none NaN; graph=True is refused."""
    from helpers import fill_module
    from stts2_mi355x.discriminators import MultiPeriodDiscriminator, MultiResSpecDiscriminator
    from stts2_mi355x.trainstep import TrainStep
    B, T = 2, 10
    dec = make_vocos(1200, 300).cuda()
    mpd = fill_module(MultiPeriodDiscriminator(), "mpd.").cuda().train()
    msd = fill_module(MultiResSpecDiscriminator(), "msd.").cuda().train()
    p0 = {k: v.detach().clone() for k, v in dec.named_parameters()}
    ins = [t.cuda() for t in _inputs(B, T)]
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
        assert not torch.equal(p.detach(), p0[k]), k
