"""GPU parity: the pitch extractor (jdc.JDCNet on the HIP plan) and log_norm against the reference's golden outputs
(tests/golden/make_golden_pitch.py), and the training step computing its own F0 / norm targets.

Bars.  fp32 / bf16x3: max|out - ref| / max(1, max|ref|) <= max(the 2-D ResNet bar of test_gpu_style.py (1e-4 /
2e-4), 4 x the fixture's own fp32-vs-fp64 difference): a GPU fp32 run cannot be asked to beat the reference's own
rounding noise.  bf16: finite and < 0.05 max|ref| (the style encoder's bf16 bar).  log_norm: 2e-6 absolute."""
import numpy as np
import pytest
import torch

from helpers import fill_module, golden
from stts2_mi355x import synth

pytestmark = pytest.mark.gpu

CASES = ((3, 1, 1), (1, 7, 1), (2, 12, 1), (2, 9, 5), (3, 130, 1))  # (B, T, num_class)
_NETS = {}


def _net(num_class):
    from stts2_mi355x.jdc import JDCNet
    if num_class not in _NETS:
        _NETS[num_class] = fill_module(JDCNet(num_class=num_class, seq_len=192), "jdc.").eval().cuda()
    return _NETS[num_class]


def _mel(B, T):
    return torch.from_numpy(np.stack([synth.normal(f"pitch:mel:{b}:{T}", (80, T)) for b in range(B)])).cuda()


def _fx(B, T, nc):
    return golden(f"pitch_B{B}_T{T}_C{nc}")


def _err(out, ref):
    return float(np.abs(out - ref).max()) / max(1.0, float(np.abs(ref).max()))


@pytest.mark.parametrize("dtype", ["fp32", "bf16x3"])
@pytest.mark.parametrize("B,T,nc", CASES)
def test_pitch_extractor(B, T, nc, dtype):
    fx = _fx(B, T, nc)
    f0, gan, pool = _net(nc)(_mel(B, T).unsqueeze(1), dtype=dtype)
    bar = max({"fp32": 1e-4, "bf16x3": 2e-4}[dtype], 4.0 * float(fx["f0_fp32_vs_fp64"]))
    outs = {"f0": f0, "pool_out": pool, "gan_feature": gan}
    for k in ("f0", "pool_out", "gan_feature"):
        assert tuple(outs[k].shape) == ((B, 256, 10, T) if k == "gan_feature" else fx[k].shape), k
        if k not in fx:
            continue
        e = _err(outs[k].cpu().numpy(), fx[k])
        print(f"pitch B={B} T={T} C={nc} {dtype} {k}: {e:.3e} (bar {bar:.1e}, ref absmax {np.abs(fx[k]).max():.3f})")
        assert e <= bar, (k, e, bar)


@pytest.mark.parametrize("B,T,nc", CASES)
def test_pitch_extractor_bf16(B, T, nc):
    fx = _fx(B, T, nc)
    f0, gan, pool = _net(nc)(_mel(B, T).unsqueeze(1), dtype="bf16")
    outs = {"f0": f0, "pool_out": pool, "gan_feature": gan}
    for k in ("f0", "pool_out", "gan_feature"):
        o = outs[k].cpu().numpy()
        assert np.isfinite(o).all(), k
        if k not in fx:
            continue
        assert o.shape == fx[k].shape
        e, scale = float(np.abs(o - fx[k]).max()), float(np.abs(fx[k]).max())
        print(f"pitch B={B} T={T} C={nc} bf16 {k}: max-abs {e:.3e} (ref absmax {scale:.3f}, {e / scale:.3e} of it)")
        assert e < 0.05 * scale, (k, e, scale)


def test_null_feature_pointers_leave_f0_bitwise():
    """stts_pitch_fwd with gan_feature = pool_out = NULL: the same f0 bits."""
    net = _net(1)
    mel = _mel(2, 12).unsqueeze(1)
    eng = net.engine("fp32")
    a, gan, pool = eng.forward(mel)
    b, g0, p0 = eng.forward(mel, features=False)
    assert g0 is None and p0 is None and gan is not None and pool is not None
    assert torch.equal(a, b)


def test_batch_invariance_fp32():
    """No cross-utterance state, no atomics: the rows of a B = 3 call are the bits of three B = 1 calls."""
    net = _net(1)
    mel = _mel(3, 130).unsqueeze(1)
    full, _, _ = net(mel)
    for b in range(3):
        one, _, _ = net(mel[b:b + 1])
        assert one.shape == (130,)
        assert torch.equal(one, full[b]), b


def test_running_statistics_make_the_pack_stale():
    from stts2_mi355x.jdc import JDCNet
    net = fill_module(JDCNet(num_class=1, seq_len=192), "jdc.").eval().cuda()
    mel = _mel(1, 7).unsqueeze(1)
    a, _, _ = net(mel)
    eng = net._engine
    net.res_block2.pre_conv[0].running_var.mul_(1.5)
    b, _, _ = net(mel)
    assert net._engine is not eng and not torch.equal(a, b)


@pytest.mark.parametrize("B,T,nc", CASES)
def test_log_norm(B, T, nc):
    from stts2_mi355x.losses import log_norm
    fx = _fx(B, T, nc)
    mel = _mel(B, T)
    out = log_norm(mel.unsqueeze(1)).squeeze(1)
    assert tuple(out.shape) == fx["n_real"].shape
    e = float(np.abs(out.cpu().numpy() - fx["n_real"]).max())
    # torch-CPU fp32 against fp64 on the same input: the reference's own error (printed with the measured value)
    x = mel.cpu()
    r32 = torch.log(torch.exp(x * 4 - 4).norm(dim=1))
    r64 = torch.log(torch.exp(x.double() * 4 - 4).norm(dim=1))
    own = float((r32.double() - r64).abs().max())
    print(f"log_norm B={B} T={T}: max-abs {e:.3e} (torch-CPU fp32 vs fp64 {own:.3e})")
    assert e <= 2e-6, e


def test_train_step_computes_its_targets():
    """TrainStep(pitch_extractor=) at the shapes of test_gpu_train_pred.py's predictor + style-encoder step:
    targets(gt) is train.py:260-262 bit for bit, and a step without explicit targets uses them."""
    from helpers import make_decoder
    from test_gpu_train_pred import _predictor
    from test_gpu_train_step import _discs, _train_inputs
    from stts2_mi355x.losses import log_norm
    from stts2_mi355x.models import StyleEncoder
    from stts2_mi355x.trainstep import TrainStep
    B, T = 2, 48
    asr, _, _, _, wav, noise = _train_inputs(B, T)
    p_en = torch.from_numpy(np.stack([synth.normal(f"tp:en:{b}:{T}", (640, T)) for b in range(B)])).cuda()
    gt = torch.from_numpy(np.stack([synth.normal(f"tp:mel:{b}:{2 * T}", (80, 2 * T)) for b in range(B)])).cuda()
    dec, _ = make_decoder("hifigan")
    mpd, msd = _discs()
    se = fill_module(StyleEncoder(dim_in=64, style_dim=128, max_conv_dim=512))
    pe = _net(1)
    step = TrainStep(dec.cuda().eval(), mpd.cuda().train(), msd.cuda().train(), predictor=_predictor().eval(),
                     style_encoder=se.cuda().eval(), pitch_extractor=pe)
    F0_real, N_real = step.targets(gt)
    with torch.no_grad():
        f0_ref = pe(gt.unsqueeze(1))[0]
        n_ref = log_norm(gt.unsqueeze(1)).squeeze(1)
    assert F0_real.shape == (B, 2 * T) and N_real.shape == (B, 2 * T)
    assert torch.equal(F0_real, f0_ref) and torch.equal(N_real, n_ref)
    out = step(asr.cuda(), None, None, None, wav.cuda(), noise=noise.cuda(), p_en=p_en, gt=gt)
    assert torch.isfinite(out["loss_F0_rec"]) and torch.isfinite(out["loss_norm_rec"])
    assert all(p.grad is None for p in pe.parameters())
    assert "pitch_extractor" not in step.opt
    from stts2_mi355x import prosody
    prosody.check_pending()  # no cooperative recurrence of this file timed out
