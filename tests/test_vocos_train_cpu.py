"""Trainable Vocos decoder, host side (no GPU): the new C-ABI entries (include/stts2_train.h: depthwise conv,
GELU, layer-scale residual, ISTFT head) exist and validate their arguments before any launch, the oracle's
autograd (oracle.decoder_vocos in fp64) reproduces the reference module's own gradients
(tests/golden/make_golden_vocos_train.py), and the ISTFT-head input recipe the GPU test shares exercises both
branches of the magnitude clip without sitting on its threshold."""
import json
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN, golden
from oracle import stts_oracle as orc
from stts2_mi355x import engine as E
from stts2_mi355x import synth
from test_vocos_cpu import make_vocos

EINVAL, EWORKSPACE = -1, -4
ENTRIES = ("stts_dwconv1d_fwd", "stts_dwconv1d_bwd", "stts_gelu_fwd", "stts_gelu_bwd", "stts_layer_scale_res_fwd",
           "stts_layer_scale_res_bwd", "stts_istft_head_fwd", "stts_istft_head_bwd")
QUERIES = ("stts_dwconv1d_bwd_workspace_bytes", "stts_layer_scale_res_bwd_workspace_bytes",
           "stts_istft_head_workspace_bytes")

HEAD_CASES = [(1200, 300, 2, 2), (1200, 300, 8, 1), (1024, 256, 33, 1)]  # (n_fft, hop, F, B)
CLIP = 100.0
NEAR = 1e-4  # relative distance of exp(h_mag) from the clip threshold below which a bin may be left out


def head_inputs(n_fft, hop, F, B):
    """The ISTFT-head test input: h [B, F, n_fft + 2] float32 (log-magnitude channels 3.0 + 2.5 randn, phase
    channels 3 randn) and the upstream gradient R [B, F hop], from fixed seeds."""
    nb = n_fft // 2 + 1
    g = torch.Generator().manual_seed(1000 * n_fft + 10 * F + B)
    mag = 3.0 + 2.5 * torch.randn(B, F, nb, generator=g)
    ph = 3.0 * torch.randn(B, F, nb, generator=g)
    R = torch.randn(B, F * hop, generator=g)
    return torch.cat([mag, ph], dim=2).float(), R.float()


def head_masks(h, n_fft):
    """(clipped, near) over the magnitude bins of h, decided in fp64 as the reference decides them."""
    nb = n_fft // 2 + 1
    e = torch.exp(h[..., :nb].double())
    return e > CLIP, (e - CLIP).abs() <= NEAR * CLIP


def _al(n):
    return (n + 255) & ~255


def test_library_exports_entries_and_queries():
    L = E.lib()
    for name in ENTRIES + QUERIES:
        assert hasattr(L, name), name
    assert L.stts_abi_version() == 5


def test_workspace_queries():
    L = E.lib()
    dw = L.stts_dwconv1d_bwd_workspace_bytes
    assert dw(2, 77, 512, 7) == _al(2 * 3 * 512 * 8 * 8)          # S = ceil(77 / 32) = 3
    assert dw(1, 100000, 100, 3) == _al(1 * 64 * 100 * 4 * 8)     # S capped at 64; C no multiple of 256
    assert dw(2, 77, 512, 6) == EINVAL                            # K even
    assert dw(2, 77, 512, 13) == EINVAL                           # K > 11
    assert dw(2, 77, 0, 7) == EINVAL and dw(2, 77, 65537, 7) == EINVAL   # C outside [1, 65536]
    assert dw(0, 77, 512, 7) == EINVAL and dw(2, 0, 512, 7) == EINVAL
    ls = L.stts_layer_scale_res_bwd_workspace_bytes
    assert ls(2, 77, 512) == _al((2 * 77 // 16) * 512 * 8)
    assert ls(2, 100000, 64) == _al(256 * 64 * 8)
    assert ls(2, 77, 0) == EINVAL and ls(0, 77, 512) == EINVAL
    hd = L.stts_istft_head_workspace_bytes
    assert hd(2, 8, 1200, 300) == _al(2 * 8 * 1200 * 4)
    assert hd(1, 33, 1024, 256) == _al(33 * 1024 * 4)
    assert hd(1, 8, 4099, 300) == EINVAL      # a prime: no two-factor split with both factors <= 64
    assert hd(1, 8, 8192, 2048) == EINVAL     # 8192 = 64 x 128: one factor above 64
    assert hd(1, 8, 1201, 301) == EINVAL      # odd n_fft
    assert hd(1, 8, 1200, 1200) == EINVAL     # hop == n_fft: no 'same' padding
    assert hd(1, 8, 1200, 301) == EINVAL      # n_fft - hop odd
    assert hd(1, 0, 1200, 300) == EINVAL and hd(0, 8, 1200, 300) == EINVAL


def test_entries_validate_before_launch():
    """Null or short arguments are refused on the host: these calls run without a device."""
    L = E.lib()
    p = 4096  # never dereferenced: every call below fails validation first
    assert L.stts_dwconv1d_fwd(None, p, p, 2, 77, 512, 7, p, None) == EINVAL
    assert L.stts_dwconv1d_fwd(p, None, p, 2, 77, 512, 7, p, None) == EINVAL
    assert L.stts_dwconv1d_fwd(p, p, p, 2, 77, 512, 7, None, None) == EINVAL
    assert L.stts_dwconv1d_fwd(p, p, p, 2, 77, 512, 8, p, None) == EINVAL
    need = L.stts_dwconv1d_bwd_workspace_bytes(2, 77, 512, 7)
    assert L.stts_dwconv1d_bwd(p, p, None, 2, 77, 512, 7, p, p, p, p, need, None) == EINVAL
    assert L.stts_dwconv1d_bwd(None, p, p, 2, 77, 512, 7, p, p, p, p, need, None) == EINVAL   # dw needs x
    assert L.stts_dwconv1d_bwd(p, None, p, 2, 77, 512, 7, p, p, p, p, need, None) == EINVAL   # dx needs w
    assert L.stts_dwconv1d_bwd(p, p, p, 2, 77, 512, 7, p, p, p, p, need - 1, None) == EWORKSPACE
    assert L.stts_dwconv1d_bwd(p, p, p, 2, 77, 512, 7, p, p, p, None, need, None) == EWORKSPACE
    assert L.stts_dwconv1d_bwd(p, p, p, 2, 77, 512, 4, p, p, p, p, need, None) == EINVAL
    assert L.stts_dwconv1d_bwd(p, p, p, 2, 77, 512, 7, None, None, None, None, 0, None) == 0  # nothing asked
    assert L.stts_gelu_fwd(None, 10, p, None) == EINVAL and L.stts_gelu_fwd(p, 10, None, None) == EINVAL
    assert L.stts_gelu_fwd(p, -1, p, None) == EINVAL and L.stts_gelu_fwd(p, 0, p, None) == 0
    assert L.stts_gelu_bwd(p, None, 10, p, None) == EINVAL and L.stts_gelu_bwd(p, p, 10, None, None) == EINVAL
    assert L.stts_layer_scale_res_fwd(p, None, p, 2, 77, 512, p, None) == EINVAL
    assert L.stts_layer_scale_res_fwd(p, p, p, 2, 77, 0, p, None) == EINVAL
    need = L.stts_layer_scale_res_bwd_workspace_bytes(2, 77, 512)
    assert L.stts_layer_scale_res_bwd(p, p, None, 2, 77, 512, p, p, p, need, None) == EINVAL
    assert L.stts_layer_scale_res_bwd(None, p, p, 2, 77, 512, p, p, p, need, None) == EINVAL  # dgamma needs x
    assert L.stts_layer_scale_res_bwd(p, p, p, 2, 77, 512, p, p, p, need - 1, None) == EWORKSPACE
    assert L.stts_layer_scale_res_bwd(p, p, p, 2, 77, 512, None, None, None, 0, None) == 0
    need = L.stts_istft_head_workspace_bytes(2, 8, 1200, 300)
    assert L.stts_istft_head_fwd(None, p, 2, 8, 1200, 300, p, p, need, None) == EINVAL
    assert L.stts_istft_head_fwd(p, None, 2, 8, 1200, 300, p, p, need, None) == EINVAL
    assert L.stts_istft_head_fwd(p, p, 2, 8, 1200, 300, None, p, need, None) == EINVAL
    assert L.stts_istft_head_fwd(p, p, 2, 8, 1200, 300, p, p, need - 1, None) == EWORKSPACE
    assert L.stts_istft_head_fwd(p, p, 2, 8, 1200, 300, p, None, need, None) == EWORKSPACE
    assert L.stts_istft_head_fwd(p, p, 2, 8, 4099, 300, p, p, need, None) == EINVAL
    assert L.stts_istft_head_bwd(p, p, None, 2, 8, 1200, 300, p, None, 0, None) == EINVAL
    assert L.stts_istft_head_bwd(p, p, p, 2, 8, 1200, 300, None, None, 0, None) == EINVAL
    assert L.stts_istft_head_bwd(p, p, p, 2, 8, 1200, 301, p, None, 0, None) == EINVAL


def test_meta_lists_the_fixture_cases():
    with open(os.path.join(GOLDEN, "meta_vocos_train.json")) as f:
        m = json.load(f)
    assert sorted(m["cases"]) == ["vocos_train_n1024_T7_B1", "vocos_train_n1200_T4_B2"]
    for name, c in m["cases"].items():
        assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < 200 << 10


def _sample_idx(numel, n=64):
    return np.arange(n) * (numel // n) if numel >= n else np.arange(n) % numel


@pytest.mark.parametrize("n_fft,hop,T,B", [(1200, 300, 4, 2), (1024, 256, 7, 1)])
def test_oracle_autograd_matches_reference_fixture(n_fft, hop, T, B):
    """Autograd through oracle.decoder_vocos in fp64 against the reference module's own backward: the loss to
    1e-10 relative, the input gradients and every parameter gradient's sum / L2 / max-abs / 64 samples to 1e-8 of
    the tensor's max |g| (floored at 1e-3 of the module's largest, the project's floor for tensors whose true
    gradient is 0, e.g. dwconv.bias feeding an InstanceNorm: those carry only fp64 rounding noise)."""
    fx = golden(f"vocos_train_n{n_fft}_T{T}_B{B}")
    dec = make_vocos(n_fft, hop)
    leaf = {k: v.detach().double().clone() for k, v in dec.state_dict().items()}
    names = [str(k) for k in fx["names"]]
    assert sorted(names) == sorted(k for k, _ in dec.named_parameters())
    for k in names:
        leaf[k].requires_grad_(True)
    ins = [torch.from_numpy(a).double().requires_grad_(True) for a in synth.decoder_inputs(B, T, tag="vocos")]
    out = orc.decoder_vocos(*ins, leaf, dict(num_layers=8, n_fft=n_fft, hop=hop))
    assert list(out.shape) == list(fx["out_shape"])
    R = torch.randn(out.shape, generator=torch.Generator().manual_seed(int(fx["r_seed"])), dtype=torch.float64)
    loss = (out * R).sum()
    loss.backward()
    assert abs(float(loss.detach()) - float(fx["loss"])) <= 1e-10 * abs(float(fx["loss"]))
    for k, t in zip(("asr", "F0_curve", "N", "s"), ins):
        ref = fx["grad_in." + k]
        assert np.abs(t.grad.numpy() - ref).max() <= 1e-8 * np.abs(ref).max(), k
    gmax = float(fx["maxabs"].max())
    for i, k in enumerate(names):
        g = leaf[k].grad.reshape(-1)
        scale = max(float(fx["maxabs"][i]), 1e-3 * gmax)
        tol = 1e-8 * scale
        assert abs(float(g.sum()) - float(fx["sum"][i])) <= tol, (k, "sum")
        assert abs(float(g.norm()) - float(fx["l2"][i])) <= tol, (k, "l2")
        assert abs(float(g.abs().max()) - float(fx["maxabs"][i])) <= tol, (k, "maxabs")
        v = g[torch.from_numpy(_sample_idx(g.numel()))].numpy()
        assert np.abs(v - fx["val"][i]).max() <= tol, (k, "samples")


@pytest.mark.parametrize("n_fft,hop,F,B", HEAD_CASES)
def test_head_input_recipe_exercises_both_clip_branches(n_fft, hop, F, B):
    h, R = head_inputs(n_fft, hop, F, B)
    assert h.shape == (B, F, n_fft + 2) and R.shape == (B, F * hop) and h.dtype == torch.float32
    clipped, near = head_masks(h, n_fft)
    frac = clipped.double().mean().item()
    assert 0.05 <= frac <= 0.60, frac
    assert near.double().mean().item() <= 1e-3
    h2, R2 = head_inputs(n_fft, hop, F, B)
    assert torch.equal(h, h2) and torch.equal(R, R2)
