"""Trainable iSTFTNet decoder, host side (no GPU): the new C-ABI entries (include/stts2_train.h: CustomSTFT
transform, reflection-pad add, exp / sin -> inverse-STFT head) exist and validate their arguments before any
launch, and the oracle's autograd (oracle.decoder_istft in fp64) reproduces the reference module's own gradients
(tests/golden/make_golden_istftnet_train.py).  None of the new entries needs a workspace, so there is no
workspace query to check."""
import json
import os
import re

import numpy as np
import pytest
import torch

from helpers import GOLDEN, ISTFT_CFG, decoder_case, golden, make_decoder
from oracle import stts_oracle as orc
from stts2_mi355x import engine as E

EINVAL = -1
ENTRIES = ("stts_cstft_fwd", "stts_padl_add_fwd", "stts_padl_add_bwd", "stts_cistft_head_fwd", "stts_cistft_head_bwd")
NO_GRAD = ["generator.m_source.l_linear.bias", "generator.m_source.l_linear.weight"]
CASES = [(4, 2), (7, 1)]  # (T, B)
# conv biases whose output goes straight into an InstanceNorm: true gradient 0
_ZERO_GRAD = re.compile(r"(\.convs1\.\d+\.bias|^encode\.conv1\.bias|^decode\.\d+\.conv1\.bias)$")


def test_library_exports_entries():
    L = E.lib()
    for name in ENTRIES:
        assert hasattr(L, name), name
    assert L.stts_abi_version() == 5


def test_entries_validate_before_launch():
    """Bad geometries are refused on the host with null pointers and without a device; so are null pointers with
    a good geometry."""
    L = E.lib()
    p = 4096  # never dereferenced: every call below fails validation first
    # (n_fft, hop): odd n_fft, n_fft 66, n_fft 2, hop 0, hop > n_fft
    for n_fft, hop in ((21, 5), (66, 5), (2, 1), (20, 0), (20, 21)):
        assert L.stts_cstft_fwd(None, None, None, 1, 100, n_fft, hop, None, None) == EINVAL, (n_fft, hop)
        assert L.stts_cistft_head_fwd(None, None, None, 1, 8, n_fft, hop, None, None) == EINVAL, (n_fft, hop)
        assert L.stts_cistft_head_bwd(None, None, None, None, 1, 8, n_fft, hop, None, None) == EINVAL, (n_fft, hop)
        assert L.stts_cistft_head_fwd(p, p, p, 1, 8, n_fft, hop, p, None) == EINVAL, (n_fft, hop)
    assert L.stts_cistft_head_fwd(None, None, None, 1, 1, 20, 5, None, None) == EINVAL      # F = 1
    assert L.stts_cistft_head_bwd(None, None, None, None, 1, 1, 20, 5, None, None) == EINVAL
    assert L.stts_cistft_head_fwd(p, p, p, 1, 1, 20, 5, p, None) == EINVAL
    assert L.stts_cistft_head_fwd(p, p, p, 0, 8, 20, 5, p, None) == EINVAL                  # B = 0
    assert L.stts_cstft_fwd(p, p, p, 0, 100, 20, 5, p, None) == EINVAL
    assert L.stts_cstft_fwd(p, p, p, 1, 0, 20, 5, p, None) == EINVAL                        # L = 0
    assert L.stts_padl_add_fwd(None, None, 1, 1, 128, None, None) == EINVAL                 # L = 1
    assert L.stts_padl_add_bwd(None, 1, 1, 128, None, None) == EINVAL
    assert L.stts_padl_add_fwd(p, p, 1, 1, 128, p, None) == EINVAL
    assert L.stts_padl_add_fwd(p, p, 1, 5, 0, p, None) == EINVAL                            # C = 0
    # good geometries (the accepted range's corners among them), a null pointer each
    for n_fft, hop in ((20, 5), (4, 1), (64, 64), (64, 1), (16, 4)):
        assert L.stts_cstft_fwd(None, p, p, 1, 100, n_fft, hop, p, None) == EINVAL
        assert L.stts_cstft_fwd(p, p, p, 1, 100, n_fft, hop, None, None) == EINVAL
        assert L.stts_cistft_head_fwd(p, None, p, 2, 8, n_fft, hop, p, None) == EINVAL
        assert L.stts_cistft_head_fwd(p, p, p, 2, 8, n_fft, hop, None, None) == EINVAL
        assert L.stts_cistft_head_bwd(p, p, p, None, 2, 8, n_fft, hop, p, None) == EINVAL
        assert L.stts_cistft_head_bwd(p, p, p, p, 2, 8, n_fft, hop, None, None) == EINVAL
    assert L.stts_padl_add_fwd(p, None, 2, 5, 7, p, None) == EINVAL
    assert L.stts_padl_add_bwd(p, 2, 5, 7, None, None) == EINVAL


def test_meta_lists_the_fixture_cases():
    with open(os.path.join(GOLDEN, "meta_istftnet_train.json")) as f:
        m = json.load(f)
    assert sorted(m["cases"]) == ["istftnet_train_T4_B2", "istftnet_train_T7_B1"]
    for name, c in m["cases"].items():
        assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < 400 << 10
        assert sorted(c["no_grad"]) == NO_GRAD


def _sample_idx(numel, n=64):
    return np.arange(n) * (numel // n) if numel >= n else np.arange(n) % numel


def oracle_leaves(dtype):
    """(state dict as leaves of `dtype`, parameter names): every parameter requires grad except m_source.l_linear.

    The reference computes the harmonic source and its STFT under torch.no_grad() (istftnet.py:544-550); the
    oracle's sine_source / stft_transform are not under no_grad, so freezing l_linear (the only trainable tensor
    that feeds them, f0_curve entering through a no_grad block already) is what makes the oracle's graph the
    reference's: `har` is then a constant there too."""
    dec, _ = make_decoder("istftnet")
    names = [k for k, _ in dec.named_parameters()]
    leaf = {k: v.detach().to(dtype).clone() for k, v in dec.state_dict().items()}
    for k in names:
        if k not in NO_GRAD:
            leaf[k].requires_grad_(True)
    return leaf, names


@pytest.mark.parametrize("T,B", CASES)
def test_oracle_autograd_matches_reference_fixture(T, B):
    """Autograd through oracle.decoder_istft in fp64 against the reference module's own backward: the loss to 1e-9
    relative, the input gradients and every parameter gradient's sum / L2 / max-abs / 64 samples to 1e-8 of the
    tensor's own max |g|.  The biases of the convs that feed an InstanceNorm directly (AdaINResBlock1.convs1,
    AdainResBlk1d.conv1: the norm cancels a per-channel shift) have a true gradient of exactly 0, so their own
    max |g| is rounding noise and no scale; for them the reference's and the oracle's values must both be zero to
    fp64 rounding, 1e-12 of the module's largest gradient (2^-53 times the ~10^4 terms of a bias sum)."""
    fx = golden(f"istftnet_train_T{T}_B{B}")
    leaf, pnames = oracle_leaves(torch.float64)
    names = [str(k) for k in fx["names"]]
    assert sorted(str(k) for k in fx["none"]) == NO_GRAD
    assert sorted(names + NO_GRAD) == sorted(pnames)
    *ins, noise = decoder_case(B, T)
    ins = [t.double().requires_grad_(True) for t in ins]
    out = orc.decoder_istft(*ins, leaf, ISTFT_CFG, noise)
    assert list(out.shape) == list(fx["out_shape"]) == [B, 1, 600 * T]
    R = torch.randn(out.shape, generator=torch.Generator().manual_seed(int(fx["r_seed"])), dtype=torch.float64)
    loss = (out * R).sum()
    loss.backward()
    assert abs(float(loss.detach()) - float(fx["loss"])) <= 1e-9 * abs(float(fx["loss"]))
    for k, t in zip(("asr", "F0_curve", "N", "s"), ins):
        ref = fx["grad_in." + k]
        assert np.abs(t.grad.numpy() - ref).max() <= 1e-8 * np.abs(ref).max(), k
    for k in NO_GRAD:
        assert leaf[k].grad is None
    gmax = float(fx["maxabs"].max())
    n_zero = 0
    for i, k in enumerate(names):
        g = leaf[k].grad.reshape(-1)
        if _ZERO_GRAD.search(k):
            n_zero += 1
            assert float(fx["maxabs"][i]) <= 1e-12 * gmax and float(g.abs().max()) <= 1e-12 * gmax, k
            continue
        tol = 1e-8 * float(fx["maxabs"][i])
        assert abs(float(g.sum()) - float(fx["sum"][i])) <= tol, (k, "sum")
        assert abs(float(g.norm()) - float(fx["l2"][i])) <= tol, (k, "l2")
        assert abs(float(g.abs().max()) - float(fx["maxabs"][i])) <= tol, (k, "maxabs")
        v = g[torch.from_numpy(_sample_idx(g.numel()))].numpy()
        assert np.abs(v - fx["val"][i]).max() <= tol, (k, "samples")
    assert n_zero == 8 * 3 + 5  # 8 AdaINResBlock1 of 3 convs1 each, encode + 4 decode blocks
