"""Training-step losses on the HIP path, drop-ins for losses.py, with autograd:

* `MultiResolutionSTFTLoss(fft_sizes, hop_sizes, win_lengths, window=torch.hann_window)`
  (losses.py:58-94): forward(x, y) = the mean over resolutions of ||y_mag - x_mag||_1 / ||y_mag||_1 with
  x_mag = (log(1e-5 + MelSpectrogram(x)) + 4) / 4 (STFTLoss, :35-55), computed by `stts_mrstft_loss`;
  backward w.r.t. x (train.py:281 `stft_loss(y_rec, wav)`: x = y_rec) by `stts_mrstft_loss_bwd`.
* `feature_loss`, `generator_loss`, `discriminator_loss`, `discriminator_TPRLS_loss`,
  `generator_TPRLS_loss` (:97-147) and the `GeneratorLoss` / `DiscriminatorLoss` modules (:149-190):
  one `stts_gan_loss` launch sequence over all the terms of a call (fixed-order fp64 sums), gradients
  by `stts_gan_loss_bwd`.  They take the reference's lists of tensors (scores [B, n], feature maps of any
  layout as long as the real and generated maps of one layer share it).
* `log_norm(x, mean=-4, std=4, dim=2)` (utils.py:48-53): the norm-consistency target of train.py:262, by
  `stts_log_norm` (no gradient: the reference calls it under no_grad).
"""
from __future__ import annotations

import ctypes

import torch
from torch import nn

from .engine import _require_device, _workspace, call
from .engine import log_norm  # noqa: F401  (utils.py:48-53, the N_real target of train.py:262)
from .training import _c

GAN_FEATURE, GAN_GEN, GAN_DISC, GAN_TPRLS = 0, 1, 2, 3


class _GanTerm(ctypes.Structure):
    _fields_ = [("a", ctypes.c_void_p), ("b", ctypes.c_void_p), ("n", ctypes.c_longlong), ("kind", ctypes.c_int)]


def _pair(r, g):
    """(r, g) as contiguous tensors with the same element order (a shared permutation of a permuted view,
    else copies): the terms are order-invariant reductions over aligned elements."""
    if r.shape != g.shape:
        raise ValueError(f"loss operands {tuple(r.shape)} and {tuple(g.shape)} differ")
    order = sorted(range(r.dim()), key=lambda d: (-r.stride(d), d))
    rp, gp = r.permute(order), g.permute(order)
    if rp.is_contiguous() and gp.is_contiguous() and rp.dtype == torch.float32 and gp.dtype == torch.float32:
        return rp, gp
    return r.float().contiguous(), g.float().contiguous()


class _GanFn(torch.autograd.Function):
    """Sum of GAN loss terms (kinds[i] over (ts[2i], ts[2i+1])) -> fp32 scalar; HIP forward and backward."""

    @staticmethod
    def forward(ctx, kinds, *ts):
        _require_device()
        n = len(kinds)
        terms = (_GanTerm * n)()
        for i, k in enumerate(kinds):
            a, b = ts[2 * i], ts[2 * i + 1]
            terms[i] = _GanTerm(a.data_ptr(), b.data_ptr(), a.numel(), int(k))
        ws, nb = _workspace("stts_gan_workspace_bytes", ts[0].device, n)  # (the backward reads it again)
        loss = torch.empty(1, dtype=torch.float64, device=ts[0].device)
        call("stts_gan_loss", terms, n, loss, ws, nb)
        ctx.save_for_backward(*ts)
        ctx.kinds, ctx.ws, ctx.nb = kinds, ws, nb
        return loss[0].to(torch.float32)

    @staticmethod
    def backward(ctx, go):
        ts = ctx.saved_tensors
        kinds = ctx.kinds
        n = len(kinds)
        need = ctx.needs_input_grad[1:]
        terms = (_GanTerm * n)()
        da = (ctypes.c_void_p * n)()
        db = (ctypes.c_void_p * n)()
        grads = []
        for i, k in enumerate(kinds):
            a, b = ts[2 * i], ts[2 * i + 1]
            terms[i] = _GanTerm(a.data_ptr(), b.data_ptr(), a.numel(), int(k))
            ga = torch.empty_like(a) if need[2 * i] else None
            gb = torch.empty_like(b) if need[2 * i + 1] else None
            da[i] = ga.data_ptr() if ga is not None else None
            db[i] = gb.data_ptr() if gb is not None else None
            grads += [ga, gb]
        g = _c(go.reshape(1))
        call("stts_gan_loss_bwd", terms, da, db, n, g, ctx.ws, ctx.nb)
        return (None, *grads)


def gan_terms(terms):
    """terms: list of (kind, a, b) -> the fp32 scalar sum, differentiable w.r.t. every a / b."""
    kinds, ts = [], []
    for kind, a, b in terms:
        a2, b2 = _pair(a, b)
        kinds.append(int(kind))
        ts += [a2, b2]
    return _GanFn.apply(tuple(kinds), *ts)


def feature_loss(fmap_r, fmap_g):
    """losses.py:97-103: 2 * sum over discriminators and layers of mean|rl - gl|."""
    return gan_terms([(GAN_FEATURE, rl, gl) for dr, dg in zip(fmap_r, fmap_g) for rl, gl in zip(dr, dg)])


def generator_loss(disc_outputs):
    """losses.py:120-128 -> (loss, [per-output losses])."""
    per = [gan_terms([(GAN_GEN, dg, dg)]) for dg in disc_outputs]
    return gan_terms([(GAN_GEN, dg, dg) for dg in disc_outputs]), per


def discriminator_loss(disc_real_outputs, disc_generated_outputs):
    """losses.py:106-117 -> (loss, r_losses, g_losses) (the per-output values as Python floats)."""
    loss = gan_terms([(GAN_DISC, dr, dg) for dr, dg in zip(disc_real_outputs, disc_generated_outputs)])
    with torch.no_grad():
        r = [float(gan_terms([(GAN_GEN, dr, dr)])) for dr in disc_real_outputs]  # mean((1 - dr)^2)
        g = [float(gan_terms([(GAN_DISC, torch.ones_like(dg), dg)])) for dg in disc_generated_outputs]
    return loss, r, g


def discriminator_TPRLS_loss(disc_real_outputs, disc_generated_outputs):
    """losses.py:131-138."""
    return gan_terms([(GAN_TPRLS, dr, dg) for dr, dg in zip(disc_real_outputs, disc_generated_outputs)])


def generator_TPRLS_loss(disc_real_outputs, disc_generated_outputs):
    """losses.py:140-147 (its loop binds the real outputs to `dg`: m = median(generated - real))."""
    return gan_terms([(GAN_TPRLS, g, r) for r, g in zip(disc_real_outputs, disc_generated_outputs)])


class GeneratorLoss(nn.Module):
    """losses.py:149-168: feature + generator + TPRLS losses over the MPD and MSD outputs, as one term list."""

    def __init__(self, mpd, msd):
        super().__init__()
        self.mpd = mpd
        self.msd = msd

    def forward(self, y, y_hat):
        y_df_hat_r, y_df_hat_g, fmap_f_r, fmap_f_g = self.mpd(y, y_hat)
        y_ds_hat_r, y_ds_hat_g, fmap_s_r, fmap_s_g = self.msd(y, y_hat)
        terms = []
        # loss_gen_s + loss_gen_f + loss_fm_s + loss_fm_f + loss_rel (the reference's sum; the sum order of
        # the fp64 term values differs from its fp32 additions only in rounding)
        terms += [(GAN_GEN, g, g) for g in y_ds_hat_g]
        terms += [(GAN_GEN, g, g) for g in y_df_hat_g]
        terms += [(GAN_FEATURE, rl, gl) for dr, dg in zip(fmap_s_r, fmap_s_g) for rl, gl in zip(dr, dg)]
        terms += [(GAN_FEATURE, rl, gl) for dr, dg in zip(fmap_f_r, fmap_f_g) for rl, gl in zip(dr, dg)]
        terms += [(GAN_TPRLS, g, r) for r, g in zip(y_df_hat_r, y_df_hat_g)]
        terms += [(GAN_TPRLS, g, r) for r, g in zip(y_ds_hat_r, y_ds_hat_g)]
        return gan_terms(terms)


class DiscriminatorLoss(nn.Module):
    """losses.py:170-190: discriminator + TPRLS losses over the MPD and MSD outputs."""

    def __init__(self, mpd, msd):
        super().__init__()
        self.mpd = mpd
        self.msd = msd

    def forward(self, y, y_hat):
        y_df_hat_r, y_df_hat_g, _, _ = self.mpd(y, y_hat)
        y_ds_hat_r, y_ds_hat_g, _, _ = self.msd(y, y_hat)
        terms = [(GAN_DISC, r, g) for r, g in zip(y_ds_hat_r, y_ds_hat_g)]
        terms += [(GAN_DISC, r, g) for r, g in zip(y_df_hat_r, y_df_hat_g)]
        terms += [(GAN_TPRLS, r, g) for r, g in zip(y_df_hat_r, y_df_hat_g)]
        terms += [(GAN_TPRLS, r, g) for r, g in zip(y_ds_hat_r, y_ds_hat_g)]
        return gan_terms(terms)


# ---------------------------------------------------------------------- multi-resolution mel loss
class _MrstftFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x2, y2, mod):
        B, L = x2.shape
        n = len(mod.fft_sizes)
        arr = lambda v: (ctypes.c_int * n)(*[int(t) for t in v])  # noqa: E731
        ffts, hops, wins = arr(mod.fft_sizes), arr(mod.hop_sizes), arr(mod.win_lengths)
        xc, yc = _c(x2), _c(y2)
        loss = torch.empty(1, dtype=torch.float64, device=xc.device)
        call("stts_mrstft_loss", xc, yc, B, L, L, ffts, hops, wins, n, mod.sample_rate, mod.n_mels, loss,
             ws=("stts_mrstft_workspace_bytes", B, L, hops, n, mod.n_mels))
        ctx.save_for_backward(xc, yc)
        ctx.mod = mod
        return loss[0].to(torch.float32)

    @staticmethod
    def backward(ctx, go):
        xc, yc = ctx.saved_tensors
        mod = ctx.mod
        if ctx.needs_input_grad[1]:
            raise NotImplementedError("MultiResolutionSTFTLoss backward w.r.t. the target y (train.py:281 "
                                      "differentiates the prediction x only)")
        if not ctx.needs_input_grad[0]:
            return None, None, None
        B, L = xc.shape
        n = len(mod.fft_sizes)
        arr = lambda v: (ctypes.c_int * n)(*[int(t) for t in v])  # noqa: E731
        ffts, hops, wins = arr(mod.fft_sizes), arr(mod.hop_sizes), arr(mod.win_lengths)
        dx = torch.empty_like(xc)
        g = _c(go.reshape(1))
        call("stts_mrstft_loss_bwd", xc, yc, B, L, L, ffts, hops, wins, n, mod.sample_rate, mod.n_mels, g, dx,
             ws=("stts_mrstft_bwd_workspace_bytes", B, L, ffts, hops, wins, n, mod.n_mels))
        return dx, None, None


class MultiResolutionSTFTLoss(nn.Module):
    def __init__(self, fft_sizes=(1024, 2048, 512), hop_sizes=(120, 240, 50), win_lengths=(600, 1200, 240),
                 window=torch.hann_window, sample_rate=24000, n_mels=128):
        super().__init__()
        assert len(fft_sizes) == len(hop_sizes) == len(win_lengths)
        if window is not torch.hann_window:
            raise NotImplementedError("the HIP log-mel uses the reference's hann window")
        self.fft_sizes, self.hop_sizes, self.win_lengths = list(fft_sizes), list(hop_sizes), list(win_lengths)
        self.sample_rate, self.n_mels = int(sample_rate), int(n_mels)

    def forward(self, x, y):
        """x (predicted), y (ground truth): [B, T] or [B, 1, T] device tensors -> 0-dim float32 tensor,
        differentiable w.r.t. x."""
        _require_device()
        if x.shape != y.shape:
            raise ValueError(f"x {tuple(x.shape)} and y {tuple(y.shape)} differ")
        L = x.shape[-1]
        dev = torch.device("cuda", torch.cuda.current_device())
        x2 = x.reshape(-1, L).to(dev)
        y2 = y.reshape(-1, L).to(dev)
        return _MrstftFn.apply(x2, y2, self)


class _SmoothL1Fn(torch.autograd.Function):
    """F.smooth_l1_loss(x, y) (beta 1, mean): stts_smooth_l1_loss / _bwd."""

    @staticmethod
    def forward(ctx, x, y):
        _require_device()
        xc, yc = _c(x), _c(y)
        if xc.shape != yc.shape:
            raise ValueError(f"smooth_l1_loss: {tuple(xc.shape)} vs {tuple(yc.shape)}")
        loss = torch.empty(1, dtype=torch.float64, device=xc.device)
        call("stts_smooth_l1_loss", xc, yc, xc.numel(), loss)
        ctx.save_for_backward(xc, yc)
        return loss[0].to(torch.float32)

    @staticmethod
    def backward(ctx, g):
        xc, yc = ctx.saved_tensors
        nx, ny = ctx.needs_input_grad
        gd = _c(g.reshape(1))
        dx = torch.empty_like(xc) if nx else None
        dy = torch.empty_like(yc) if ny else None
        call("stts_smooth_l1_loss_bwd", xc, yc, xc.numel(), gd, dx, dy)
        return dx, dy


def smooth_l1_loss(x, y):
    """F.smooth_l1_loss(x, y) as train.py:269-270 calls it (loss_F0_rec = smooth_l1(F0_real, F0_fake) / 10,
    loss_norm_rec = smooth_l1(N_real, N_fake))."""
    return _SmoothL1Fn.apply(x, y)


class _S2SLossFn(torch.autograd.Function):
    """loss_s2s (train.py:301-304): value and gradient in one launch (stts_s2s_loss)."""

    @staticmethod
    def forward(ctx, pred, texts, ln):
        _require_device()
        pc = pred if pred.stride(-1) == 1 and pred.dtype == torch.float32 else _c(pred)
        B, T, K = pc.shape
        tok = texts.to(device=pc.device, dtype=torch.int64)
        if tok.stride(-1) != 1:
            tok = tok.contiguous()
        loss = torch.empty(1, dtype=torch.float64, device=pc.device)
        call("stts_s2s_loss", pc, pc.stride(0), pc.stride(1), B, T, K, tok, tok.stride(0), ln, loss, None, None,
             ws=("stts_s2s_loss_workspace_bytes", B))
        ctx.save_for_backward(pc, tok, ln)
        return loss[0].to(torch.float32)

    @staticmethod
    def backward(ctx, g):
        pc, tok, ln = ctx.saved_tensors
        B, T, K = pc.shape
        loss = torch.empty(1, dtype=torch.float64, device=pc.device)
        dz = torch.empty(B, T, K, dtype=torch.float32, device=pc.device)
        call("stts_s2s_loss", pc, pc.stride(0), pc.stride(1), B, T, K, tok, tok.stride(0), ln, loss, dz,
             _c(g.reshape(1)), ws=("stts_s2s_loss_workspace_bytes", B))
        return dz, None, None


def s2s_loss(s2s_pred, texts, input_lengths):
    """train.py:301-304: mean over the batch of cross_entropy(s2s_pred[b, :len_b], texts[b, :len_b]).  s2s_pred
    [B, T, n_token] with T >= max(len); texts [B, >= max(len)] integer tokens inside the table (IndexError
    otherwise, before any launch)."""
    ln_host = torch.as_tensor(input_lengths).detach().cpu().to(torch.int64)
    tk = torch.as_tensor(texts).detach().cpu()
    B, T, K = s2s_pred.shape
    if ln_host.numel() != B or int(ln_host.max()) > min(T, tk.shape[1]) or int(ln_host.min()) < 0:
        raise ValueError(f"s2s_loss: lengths {ln_host.tolist()} for logits {tuple(s2s_pred.shape)}, "
                         f"texts {tuple(tk.shape)}")
    for b in range(B):
        row = tk[b, :int(ln_host[b])]
        if row.numel() and (int(row.min()) < 0 or int(row.max()) >= K):
            raise IndexError(f"s2s_loss: token indices must lie in [0, {K})")
    ln = ln_host.to(device=s2s_pred.device, dtype=torch.int32)
    return _S2SLossFn.apply(s2s_pred, texts, ln)


class _MonoLossFn(torch.autograd.Function):
    """loss_mono (train.py:306): value and gradient in one launch (stts_mono_loss)."""

    @staticmethod
    def forward(ctx, attn, mono):
        _require_device()
        ac, mc = _c(attn), _c(mono)
        if ac.shape != mc.shape:
            raise ValueError(f"mono_loss: {tuple(ac.shape)} vs {tuple(mc.shape)}")
        loss = torch.empty(1, dtype=torch.float64, device=ac.device)
        call("stts_mono_loss", ac, mc, ac.numel(), loss, None, None)
        ctx.save_for_backward(ac, mc)
        return loss[0].to(torch.float32)

    @staticmethod
    def backward(ctx, g):
        ac, mc = ctx.saved_tensors
        loss = torch.empty(1, dtype=torch.float64, device=ac.device)
        da = torch.empty_like(ac)
        call("stts_mono_loss", ac, mc, ac.numel(), loss, da, _c(g.reshape(1)))
        return da, (-da if ctx.needs_input_grad[1] else None)


def mono_loss(s2s_attn, s2s_attn_mono):
    """train.py:306: F.l1_loss(s2s_attn, s2s_attn_mono) * 10."""
    return _MonoLossFn.apply(s2s_attn, s2s_attn_mono)
