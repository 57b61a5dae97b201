"""Training-step layers on the HIP path: conv1d, AdaIN1d + Snake /
LeakyReLU, the style Linear, weight norm, and the AdaINResBlock1 built from them, each a
`torch.autograd.Function` whose forward and backward both run as HIP kernels behind the C-ABI.

train.py:272-327 backpropagates the discriminator and generator losses through every nn.Conv1d of
the decoder (Modules/hifigan.py) and the discriminators (Modules/discriminators.py).  `conv1d` is
that layer as a `torch.autograd.Function` over the C-ABI: forward = `stts_conv1d_fwd` (the conv
engine), backward = `stts_conv1d_bwd` (dx on the conv engine as the transposed conv of dy; dw and
db as fp32 MFMA row-slice sums reduced in fixed order).  `Conv1d` is the drop-in nn.Conv1d
(groups = 1, padding_mode 'zeros') whose forward and backward both run there.

Torch tensors are [B, C, L]; the kernels take frames [B][L][C], so the wrapper transposes at the
boundary (plumbing, not compute).
"""
from __future__ import annotations

import ctypes
import math

import torch
from torch import nn

from .engine import _require_device, _workspace, call  # noqa: F401  (_workspace: texttrain, losses and tests import it)

# bf16x3: the split-operand mode (fp32 frames, forward / dx operands as bf16 hi + lo, three MFMAs; dw in fp32)
_DT = {"fp32": 0, "bf16": 1, "bf16x3": 2}
# algorithmic conv work of the autograd path (measurement: tools/bench_train_step.py): 2 B Lq Cout Cin K flops per
# conv forward, the same again per dx and per dw (the transposed conv: 2 B Lin Cin Cout K)
CONV_FLOPS = {"on": False, "fwd": 0.0, "bwd": 0.0}


def _count(kind, flops):
    if CONV_FLOPS["on"]:
        CONV_FLOPS[kind] += flops


def out_length(Lin: int, K: int, stride: int, pad: int, dil: int) -> int:
    return (Lin + 2 * pad - dil * (K - 1) - 1) // stride + 1


class _Conv1dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias, stride, pad, dil, dtype, res=None, scale=1.0, act=None):
        """x: frames [B, Lin, Cin] -> y frames [B, Lq, Cout] (+ res, fp32 frames [B, Lq, Cout]);
        act = a leaky-ReLU slope applied in the conv epilogue (stts_conv1d_fwd_act), or None"""
        _require_device()
        B, Lin, Cin = x.shape
        Cout, Cin_w, K = w.shape
        if Cin_w != Cin:
            raise ValueError(f"weight {tuple(w.shape)} does not take {Cin} input channels")
        Lq = out_length(Lin, K, stride, pad, dil)
        dt = _DT[dtype]
        xf = x.detach().to(torch.float32).contiguous()
        wc = w.detach().to(torch.float32).contiguous()
        bc = bias.detach().to(torch.float32).contiguous() if bias is not None else None
        geo = (B, Lin, Cin, Cout, K, stride, dil, pad, Lq)
        ws = ("stts_conv1d_fwd_workspace_bytes", dt, *geo)
        y = torch.empty(B, Lq, Cout, dtype=torch.float32, device=x.device)
        ctx.scale = float(scale)
        ctx.act = act
        if act is not None:
            if res is not None or scale != 1.0:
                raise ValueError("conv1d_frames: the fused leaky ReLU takes no residual / scale")
            call("stts_conv1d_fwd_act", dt, xf, wc, bc, *geo, act, y, ws=ws)
        elif res is not None and dt != 0:
            # the residual epilogue of stts_conv1d_fwd_res is fp32-only: bf16 runs add it in a second pass
            call("stts_conv1d_fwd", dt, xf, wc, bc, *geo, y, ws=ws)
            rc = res.detach().to(torch.float32).contiguous()
            xs = (ctypes.c_void_p * 2)(y.data_ptr(), rc.data_ptr())
            call("stts_sum_div", xs, 2, y.numel(), 1.0 / scale, y)
        elif res is not None or scale != 1.0:
            rc = res.detach().to(torch.float32).contiguous() if res is not None else None
            call("stts_conv1d_fwd_res", dt, xf, wc, bc, rc, scale, *geo, y, ws=ws)
        else:
            call("stts_conv1d_fwd", dt, xf, wc, bc, *geo, y, ws=ws)
        ctx.save_for_backward(xf, wc, y if act is not None else None)
        ctx.geo = (*geo, dt, bias is not None)
        _count("fwd", 2.0 * B * Lq * Cout * Cin * K)
        return y

    @staticmethod
    def backward(ctx, gy):
        xf, wc, ya = ctx.saved_tensors
        B, Lin, Cin, Cout, K, stride, dil, pad, Lq, dt, has_bias = ctx.geo
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        if ctx.scale != 1.0:
            gy = gy * ctx.scale
        dyf = gy.detach().to(torch.float32).contiguous()
        if ctx.act is not None:  # through the fused leaky ReLU, on its output (the slope keeps the sign)
            dpre = torch.empty_like(dyf)
            call("stts_leaky_relu_bwd", ya, dyf, ya.numel(), ctx.act, dpre)
            dyf = dpre
        dev = dyf.device
        dx = torch.empty(B, Lin, Cin, dtype=torch.float32, device=dev) if need_x else None
        dw = torch.empty(Cout, Cin, K, dtype=torch.float32, device=dev) if need_w else None
        db = torch.empty(Cout, dtype=torch.float32, device=dev) if (need_b and has_bias) else None
        call("stts_conv1d_bwd", dt, xf, wc, dyf, B, Lin, Cin, Cout, K, stride, dil, pad, Lq, dx, dw, db,
             ws=("stts_conv1d_bwd_workspace_bytes", dt, B, Lin, Cin, Cout, K, stride, dil, pad, Lq))
        _count("bwd", 2.0 * B * Lq * Cout * Cin * K * ((dx is not None) + (dw is not None)))
        return dx, dw, db, None, None, None, None, (gy if ctx.needs_input_grad[7] else None), None, None


def conv1d(x, weight, bias=None, stride=1, padding=0, dilation=1, dtype="fp32"):
    """torch.nn.functional.conv1d (groups 1, zero padding) with forward and backward on the HIP
    conv engines.  dtype 'bf16' runs the forward and dx with bf16 operands (fp32 accumulation);
    dw / db are always fp32."""
    if dtype not in _DT:
        raise ValueError(f"dtype {dtype!r}: expected one of {list(_DT)}")
    return conv1d_frames(x.transpose(1, 2), weight, bias, stride, padding, dilation, dtype).transpose(1, 2)


# True: stride-2 convs run as stride-1 convs over phase-folded frames (see _fold_strided).  Off by default:
# on the config-5 step it measured slower (103.9 vs 99.3 ms, profiles/r03_bench_train_fold_ab.txt): the
# folded dx has 192 output channels and the per-call weight gather adds launches.  Tests compare both paths.
FOLD_STRIDED = False
# the discriminators' conv -> leaky_relu(0.1) pairs as one launch (stts_conv1d_fwd_act); False = separate passes
FUSE_LRELU = True
_FOLD_MAPS = {}


def _fold_map(K, stride, pad):
    """(K', pad', [(phase, k', t)]) of the stride-1 conv equivalent to a stride-`stride` one: input row
    stride q + t - pad = stride (q + s') + ph, k' = s' - s'_min."""
    key = (K, stride, pad)
    if key not in _FOLD_MAPS:
        js = [t - pad for t in range(K)]
        smin, smax = min(j // stride for j in js), max(j // stride for j in js)
        _FOLD_MAPS[key] = (smax - smin + 1, -smin, [(j % stride, j // stride - smin, t) for t, j in enumerate(js)])
    return _FOLD_MAPS[key]


def _fold_strided(x, weight, stride, padding):
    """A Conv1d(stride s, dilation 1) y[q] = sum_t w[t] x[s q + t - pad] is the stride-1 conv
    y[q] = sum_k' w'[k'] x'[q + k' - pad'] over the frames x'[m] = (x[s m], x[s m + 1], ..., x[s m + s - 1])
    (a free view of the contiguous frames [B, L, C] as [B, L / s, s C], rows padded to a multiple of s),
    with w'[k'][(ph, ci)] = w[t] where s (k' - pad') + ph = t - pad (zero elsewhere).  So the MSD / MPD
    strided convs run on the stride-1 engines (full MFMA columns at N = 32, stride-1 dx and dw) instead of the
    strided igemm tile (64 rows x 128 columns).  Autograd goes through the view and the weight gather."""
    B, Lin, Cin = x.shape
    Cout, _, K = weight.shape
    K2, pad2, taps = _fold_map(K, stride, padding)
    L2 = -(-Lin // stride)
    if L2 * stride != Lin:
        x = torch.nn.functional.pad(x, (0, 0, 0, L2 * stride - Lin))
    x2 = x.reshape(B, L2, stride * Cin)
    w2 = weight.new_zeros(Cout, stride, Cin, K2)
    for ph, k2, t in taps:
        w2[:, ph, :, k2] = weight[:, :, t]
    return x2, w2.reshape(Cout, stride * Cin, K2), pad2


def conv1d_frames(x, weight, bias=None, stride=1, padding=0, dilation=1, dtype="fp32", residual=None, scale=1.0,
                  act_slope=None):
    """conv1d on frames tensors: x [B, Lin, Cin] -> [B, Lq, Cout] (the kernels' native layout);
    `residual` (frames [B, Lq, Cout], fp32 runs) is added and the sum multiplied by `scale` in the
    conv epilogue; `act_slope`: leaky_relu(., act_slope) applied in the epilogue instead (FUSE_LRELU)."""
    if dtype not in _DT:
        raise ValueError(f"dtype {dtype!r}: expected one of {list(_DT)}")
    if residual is None and scale != 1.0:
        raise ValueError("conv1d_frames: `scale` applies to the residual sum; pass a residual or scale 1")
    stride, padding, dilation = int(stride), int(padding), int(dilation)
    if FOLD_STRIDED and stride == 2 and dilation == 1 and residual is None:
        Lq = out_length(x.shape[1], weight.shape[-1], stride, padding, 1)
        x2, w2, pad2 = _fold_strided(x, weight, stride, padding)
        y = _Conv1dFn.apply(x2, w2, bias, 1, pad2, 1, dtype, None, 1.0, act_slope)
        return y[:, :Lq] if y.shape[1] != Lq else y
    return _Conv1dFn.apply(x, weight, bias, stride, padding, dilation, dtype, residual, float(scale), act_slope)


class Conv1d(nn.Conv1d):
    """nn.Conv1d drop-in (same parameters and state dict) computing on the HIP path."""

    def __init__(self, *args, dtype_compute: str = "fp32", **kw):
        super().__init__(*args, **kw)
        if self.groups != 1 or self.padding_mode != "zeros" or isinstance(self.padding, str):
            raise NotImplementedError("HIP Conv1d: groups 1, integer zero padding")
        self.dtype_compute = dtype_compute

    def forward(self, x):
        return conv1d(x, self.weight, self.bias, self.stride[0], self.padding[0], self.dilation[0],
                      self.dtype_compute)


class _ConvT1dFn(torch.autograd.Function):
    """ConvTranspose1d on frames: x [B, Lin, Cin] -> [B, Lout, Cout], w [Cin, Cout, K]."""

    @staticmethod
    def forward(ctx, x, w, bias, stride, pad, out_pad, dtype):
        _require_device()
        B, Lin, Cin = x.shape
        Cin_w, Cout, K = w.shape
        if Cin_w != Cin:
            raise ValueError(f"weight {tuple(w.shape)} does not take {Cin} input channels")
        Lout = (Lin - 1) * stride - 2 * pad + K + out_pad
        dt = _DT[dtype]
        xf, wc, bc = _c(x), _c(w), _c(bias)
        y = torch.empty(B, Lout, Cout, dtype=torch.float32, device=x.device)
        call("stts_conv_transpose1d_fwd", dt, xf, wc, bc, B, Lin, Cin, Cout, K, stride, pad, Lout, y,
             ws=("stts_conv_transpose1d_workspace_bytes", dt, B, Lin, Cin, Cout, K, stride, pad, Lout))
        ctx.save_for_backward(xf, wc)
        ctx.geo = (B, Lin, Cin, Cout, K, stride, pad, Lout, dt, bias is not None)
        _count("fwd", 2.0 * B * Lin * Cin * Cout * K)
        return y

    @staticmethod
    def backward(ctx, gy):
        xf, wc = ctx.saved_tensors
        B, Lin, Cin, Cout, K, stride, pad, Lout, dt, has_bias = ctx.geo
        nx, nw, nbias = ctx.needs_input_grad[:3]
        dy = _c(gy)
        dx = torch.empty_like(xf) if nx else None
        dw = torch.empty_like(wc) if nw else None
        db = torch.empty(Cout, dtype=torch.float32, device=dy.device) if (nbias and has_bias) else None
        call("stts_conv_transpose1d_bwd", dt, xf, wc, dy, B, Lin, Cin, Cout, K, stride, pad, Lout, dx, dw, db,
             ws=("stts_conv_transpose1d_workspace_bytes", dt, B, Lin, Cin, Cout, K, stride, pad, Lout))
        _count("bwd", 2.0 * B * Lin * Cin * Cout * K * ((dx is not None) + (dw is not None)))
        return dx, dw, db, None, None, None, None


def conv_transpose1d_frames(x, weight, bias=None, stride=1, padding=0, output_padding=0, dtype="fp32"):
    """F.conv_transpose1d (groups 1, dilation 1) on frames [B, Lin, Cin] -> [B, Lout, Cout]."""
    if dtype not in _DT:
        raise ValueError(f"dtype {dtype!r}: expected one of {list(_DT)}")
    return _ConvT1dFn.apply(x, weight, bias, int(stride), int(padding), int(output_padding), dtype)


def conv_transpose1d(x, weight, bias=None, stride=1, padding=0, output_padding=0, dtype="fp32"):
    """F.conv_transpose1d on [B, C, L] tensors with forward and backward on the HIP path."""
    return conv_transpose1d_frames(x.transpose(1, 2), weight, bias, stride, padding, output_padding,
                                   dtype).transpose(1, 2)


ACT_NONE, ACT_SNAKE, ACT_LRELU = 0, 1, 2


def _c(t):
    """t as a detached, contiguous float32 tensor (None stays None): what the kernels read."""
    return t.detach().to(torch.float32).contiguous() if t is not None else None


class _LinearFn(torch.autograd.Function):
    """nn.Linear on the device (stts_linear_fwd / stts_linear_bwd): s [B, K], W [N, K] -> [B, N]."""

    @staticmethod
    def forward(ctx, s, W, b):
        _require_device()
        B, K = s.shape
        N = W.shape[0]
        sc, Wc, bc = _c(s), _c(W), _c(b)
        h = torch.empty(B, N, dtype=torch.float32, device=s.device)
        call("stts_linear_fwd", sc, Wc, bc, B, K, N, h)
        ctx.save_for_backward(sc, Wc)
        ctx.has_b = b is not None
        return h

    @staticmethod
    def backward(ctx, dh):
        sc, Wc = ctx.saved_tensors
        B, K = sc.shape
        N = Wc.shape[0]
        dh = _c(dh)
        ns, nw, nb = ctx.needs_input_grad
        ds = torch.empty_like(sc) if ns else None
        dW = torch.empty_like(Wc) if nw else None
        db = torch.empty(N, dtype=torch.float32, device=dh.device) if (nb and ctx.has_b) else None
        call("stts_linear_bwd", sc, Wc, dh, B, K, N, ds, dW, db)
        return ds, dW, db


class _AdaINActFn(torch.autograd.Function):
    """AdaIN1d (InstanceNorm + (1 + gamma), beta) + activation on frames [B, L, C]; gb [B, 2C]."""

    @staticmethod
    def forward(ctx, x, gb, alpha, act):
        _require_device()
        B, L, C = x.shape
        xc, gbc, ac = _c(x), _c(gb), _c(alpha.reshape(-1)) if alpha is not None else None
        y = torch.empty_like(xc)
        mr = torch.empty(B, C, 2, dtype=torch.float32, device=x.device)
        call("stts_adain_act_fwd", xc, gbc, ac, act, B, L, C, y, mr, ws=("stts_adain_act_workspace_bytes", B, L, C))
        ctx.save_for_backward(xc, gbc, ac if ac is not None else xc.new_empty(0), mr)
        ctx.act, ctx.alpha_shape = act, (alpha.shape if alpha is not None else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        xc, gbc, ac, mr = ctx.saved_tensors
        act = ctx.act
        B, L, C = xc.shape
        dy = _c(dy)
        nx, ngb, na = ctx.needs_input_grad[:3]
        dx = torch.empty_like(xc) if nx else None
        dgb = torch.empty_like(gbc) if ngb else None
        da = torch.empty(C, dtype=torch.float32, device=dy.device) if (na and act == ACT_SNAKE) else None
        call("stts_adain_act_bwd", xc, gbc, ac if act == ACT_SNAKE else None, act, mr, dy, B, L, C, dx, dgb, da,
             ws=("stts_adain_act_workspace_bytes", B, L, C))
        return dx, dgb, (da.reshape(ctx.alpha_shape) if da is not None else None), None


class _WeightNormFn(torch.autograd.Function):
    """w = g v / ||v|| (norm over all dims but 0): stts_weight_norm / stts_weight_norm_bwd."""

    @staticmethod
    def forward(ctx, g, v):
        _require_device()
        gc, vc = _c(g), _c(v)
        d0 = vc.shape[0]
        w = torch.empty_like(vc)
        call("stts_weight_norm", gc, vc, d0, vc.numel() // d0, w)
        ctx.save_for_backward(gc, vc)
        ctx.g_shape = g.shape
        return w

    @staticmethod
    def backward(ctx, dw):
        gc, vc = ctx.saved_tensors
        d0 = vc.shape[0]
        dw = _c(dw)
        dg = torch.empty(d0, dtype=torch.float32, device=dw.device)
        dv = torch.empty_like(vc)
        call("stts_weight_norm_bwd", gc, vc, dw, d0, vc.numel() // d0, dg, dv)
        return dg.reshape(ctx.g_shape), dv


def linear(s, W, b=None):
    return _LinearFn.apply(s, W, b)


def adain_act(x, s, fc_weight, fc_bias, alpha=None, act=ACT_NONE):
    """AdaIN1d(style) on frames x [B, L, C] followed by `act` (Snake needs alpha [C] or [1, C, 1])."""
    return _AdaINActFn.apply(x, linear(s, fc_weight, fc_bias), alpha, int(act))


def weight_norm(g, v):
    return _WeightNormFn.apply(g, v)


class _WNConv(nn.Module):
    """weight_norm(nn.Conv1d) parameter layout (weight_g [Cout, 1, 1], weight_v, bias)."""

    def __init__(self, cin, cout, k, dilation=1, padding=0):
        super().__init__()
        self.weight_g = nn.Parameter(torch.ones(cout, 1, 1))
        self.weight_v = nn.Parameter(torch.randn(cout, cin, k) * 0.02)
        self.bias = nn.Parameter(torch.zeros(cout))
        self.dilation, self.padding = dilation, padding


class _AdaIN(nn.Module):
    def __init__(self, style_dim, C):
        super().__init__()
        self.fc = nn.Linear(style_dim, 2 * C)


class AdaINResBlock1(nn.Module):
    """Trainable Modules/hifigan.py:26-80 AdaINResBlock1 (same parameter names: convs1/convs2 weight-normed,
    adain1/adain2 .fc, alpha1/alpha2), forward and backward on the HIP kernels:
    for each dilation d: xt = Snake(AdaIN1(x)); xt = convs1(xt); xt = Snake(AdaIN2(xt)); xt = convs2(xt);
    x = xt + x.  `forward(x, s)` takes x [B, C, L]; `forward_frames(x, s)` frames [B, L, C]."""

    def __init__(self, channels, kernel_size=3, dilation=(1, 3, 5), style_dim=64):
        super().__init__()
        self.kernel_size, self.dilation = kernel_size, tuple(dilation)
        self.convs1 = nn.ModuleList([_WNConv(channels, channels, kernel_size, d, (kernel_size * d - d) // 2)
                                     for d in dilation])
        self.convs2 = nn.ModuleList([_WNConv(channels, channels, kernel_size, 1, (kernel_size - 1) // 2)
                                     for _ in dilation])
        self.adain1 = nn.ModuleList([_AdaIN(style_dim, channels) for _ in dilation])
        self.adain2 = nn.ModuleList([_AdaIN(style_dim, channels) for _ in dilation])
        self.alpha1 = nn.ParameterList([nn.Parameter(torch.ones(1, channels, 1)) for _ in dilation])
        self.alpha2 = nn.ParameterList([nn.Parameter(torch.ones(1, channels, 1)) for _ in dilation])

    def forward_frames(self, x, s):
        return resblock1_frames(self, x, s)

    def forward(self, x, s):
        return self.forward_frames(x.transpose(1, 2), s).transpose(1, 2)


def resblock1_frames(m, x, s, dtype="fp32"):
    """AdaINResBlock1.forward (hifigan.py:65-74) on frames x [B, L, C] for any module with the reference's
    parameter layout (training.AdaINResBlock1 or the decoder's params.AdaINResBlock1):
    for each dilation: xt = Snake(AdaIN1(x)); xt = convs1(xt); xt = Snake(AdaIN2(xt)); x = convs2(xt) + x."""
    for c1, c2, n1, n2, a1, a2 in zip(m.convs1, m.convs2, m.adain1, m.adain2, m.alpha1, m.alpha2):
        xt = adain_act(x, s, n1.fc.weight, n1.fc.bias, a1, ACT_SNAKE)
        xt = conv1d_frames(xt, weight_norm(c1.weight_g, c1.weight_v), c1.bias, 1, c1.padding, c1.dilation, dtype)
        xt = adain_act(xt, s, n2.fc.weight, n2.fc.bias, a2, ACT_SNAKE)
        x = conv1d_frames(xt, weight_norm(c2.weight_g, c2.weight_v), c2.bias, 1, c2.padding, c2.dilation, dtype,
                          residual=x)  # x = xt + x in convs2's epilogue
    return x


class _PoolFn(torch.autograd.Function):
    """AdainResBlk1d.pool: depthwise ConvTranspose1d(C, C, 3, 2, 1, output_padding 1) on frames."""

    @staticmethod
    def forward(ctx, x, w, bias):
        _require_device()
        B, Lin, C = x.shape
        xc, wc, bc = _c(x), _c(w).reshape(C, 3), _c(bias)
        y = torch.empty(B, 2 * Lin, C, dtype=torch.float32, device=x.device)
        call("stts_pool_fwd", xc, wc, bc, B, Lin, C, y)
        ctx.save_for_backward(xc, wc)
        ctx.w_shape, ctx.has_b = w.shape, bias is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        xc, wc = ctx.saved_tensors
        B, Lin, C = xc.shape
        dy = _c(gy)
        nx, nw, nb = ctx.needs_input_grad
        dx = torch.empty_like(xc) if nx else None
        dw = torch.empty(C, 3, dtype=torch.float32, device=dy.device) if nw else None
        db = torch.empty(C, dtype=torch.float32, device=dy.device) if (nb and ctx.has_b) else None
        call("stts_pool_bwd", xc, wc, dy, B, Lin, C, dx, dw, db, ws=("stts_pool_workspace_bytes", B, Lin, C))
        return dx, (dw.reshape(ctx.w_shape) if dw is not None else None), db


class _Up2Fn(torch.autograd.Function):
    """nearest x2 upsample of frames (UpSample1d 'half')."""

    @staticmethod
    def forward(ctx, x):
        _require_device()
        B, Lin, C = x.shape
        xc = _c(x)
        y = torch.empty(B, 2 * Lin, C, dtype=torch.float32, device=x.device)
        call("stts_upsample2", xc, B, Lin, C, y)
        ctx.shape = (B, Lin, C)
        return y

    @staticmethod
    def backward(ctx, gy):
        B, Lin, C = ctx.shape
        dy = _c(gy)
        dx = torch.empty(B, Lin, C, dtype=torch.float32, device=dy.device)
        call("stts_upsample2_bwd", dy, B, Lin, C, dx)
        return dx


class _WNConvT(nn.Module):
    """weight_norm(nn.ConvTranspose1d(C, C, 3, groups=C)) parameter layout (AdainResBlk1d.pool)."""

    def __init__(self, C):
        super().__init__()
        self.weight_g = nn.Parameter(torch.ones(C, 1, 1))
        self.weight_v = nn.Parameter(torch.randn(C, 1, 3) * 0.3)
        self.bias = nn.Parameter(torch.zeros(C))


class AdainResBlk1d(nn.Module):
    """Trainable Modules/hifigan.py:359-403 AdainResBlk1d (the decoder's encode / decode blocks; same
    parameter names), forward and backward on the HIP kernels:
    r = conv2(LReLU(AdaIN2(conv1(pool(LReLU(AdaIN1(x)))))), sc = conv1x1(up2(x)),
    out = (r + sc) / sqrt(2) (the sum and the scale ride in conv2's epilogue).  Dropout p = 0 (the
    decoder's setting)."""

    def __init__(self, dim_in, dim_out, style_dim=64, upsample="none"):
        super().__init__()
        self.upsample = upsample not in ("none", False, None)
        self.learned_sc = dim_in != dim_out
        self.conv1 = _WNConv(dim_in, dim_out, 3, 1, 1)
        self.conv2 = _WNConv(dim_out, dim_out, 3, 1, 1)
        self.norm1 = _AdaIN(style_dim, dim_in)
        self.norm2 = _AdaIN(style_dim, dim_out)
        if self.learned_sc:
            self.conv1x1 = _WNConv(dim_in, dim_out, 1, 1, 0)
            self.conv1x1.bias = None
        if self.upsample:
            self.pool = _WNConvT(dim_in)

    def forward_frames(self, x, s):
        return adain_resblk1d_frames(self, x, s)

    def forward(self, x, s):
        return self.forward_frames(x.transpose(1, 2), s).transpose(1, 2)


def conv1d_chunked(x, weight, bias, padding, dtype, chunk, residual=None, scale=1.0):
    """A stride-1 conv1d_frames summed in blocks of `chunk` channels: output channels in blocks (concatenated), the
    input channels of each in blocks whose partial convs are added in order (sum_div), then (y + residual) * scale.
    The fp32 engine adds the C_in K products of an output in one chain (3,270 terms for the front-end's
    1090-channel k3 convs), and its dx the C_out K products; blocks of 512 halve the rounding of both."""
    Cout, Cin, _ = weight.shape
    cols = []
    for o0 in range(0, Cout, chunk):
        wo = weight[o0:o0 + chunk]
        bo = bias[o0:o0 + chunk] if bias is not None else None
        parts = [conv1d_frames(x[..., c0:c0 + chunk], wo[:, c0:c0 + chunk], bo if c0 == 0 else None, 1, padding, 1,
                               dtype) for c0 in range(0, Cin, chunk)]
        cols.append(parts[0] if len(parts) == 1 else sum_div(parts))
    y = cols[0] if len(cols) == 1 else torch.cat(cols, dim=-1)
    return y if residual is None else sum_div([y, residual], 1.0 / scale)


def adain_resblk1d_frames(m, x, s, dtype="fp32", kchunk=0):
    """AdainResBlk1d.forward (hifigan.py:384-403, dropout p = 0) on frames x [B, L, C_in] for any module with
    the reference's parameter layout (training.AdainResBlk1d or params.AdainResBlk1d):
    out = (conv2(LReLU(AdaIN2(conv1(pool(LReLU(AdaIN1(x))))))) + conv1x1(up2(x))) / sqrt(2), the sum and the
    scale in conv2's epilogue.  kchunk > 0: the three convs through conv1d_chunked (fp32 accuracy)."""
    up = m.upsample if isinstance(getattr(m, "upsample", None), bool) else m.upsample_type != "none"
    # nn.Dropout(dropout_p) before each conv in train mode (models.py:335, 358-367; the predictor's blocks)
    # (the reference's AdainResBlk1d keeps only self.dropout = nn.Dropout(p), models.py:335: read its p then)
    p_drop = getattr(m, "dropout_p", None)
    if p_drop is None:
        p_drop = getattr(getattr(m, "dropout", None), "p", 0.0)
    p_drop = float(p_drop or 0.0) if m.training else 0.0
    r = adain_act(x, s, m.norm1.fc.weight, m.norm1.fc.bias, None, ACT_LRELU)
    if up:
        r = _PoolFn.apply(r, _wn_w(m.pool), m.pool.bias)
    c1, c2 = m.conv1, m.conv2
    if kchunk:
        r = conv1d_chunked(dropout(r, p_drop), _wn_w(c1), c1.bias, 1, dtype, kchunk)
        r = dropout(adain_act(r, s, m.norm2.fc.weight, m.norm2.fc.bias, None, ACT_LRELU), p_drop)
        sc = _Up2Fn.apply(x) if up else x
        if m.learned_sc:
            sc = conv1d_chunked(sc, _wn_w(m.conv1x1), None, 0, dtype, kchunk)
        return conv1d_chunked(r, _wn_w(c2), c2.bias, 1, dtype, kchunk, residual=sc, scale=1 / math.sqrt(2))
    r = conv1d_frames(dropout(r, p_drop), _wn_w(c1), c1.bias, 1, 1, dtype=dtype)
    r = dropout(adain_act(r, s, m.norm2.fc.weight, m.norm2.fc.bias, None, ACT_LRELU), p_drop)
    sc = _Up2Fn.apply(x) if up else x
    if m.learned_sc:
        sc = conv1d_frames(sc, _wn_w(m.conv1x1), None, 1, 0, dtype=dtype)
    return conv1d_frames(r, _wn_w(c2), c2.bias, 1, 1, dtype=dtype, residual=sc,
                         scale=1 / math.sqrt(2))


class _LReLUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, slope):
        _require_device()
        xc = _c(x)
        y = torch.empty_like(xc)
        call("stts_leaky_relu", xc, xc.numel(), slope, y)
        ctx.save_for_backward(y)
        ctx.slope = slope
        return y

    @staticmethod
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        dy = _c(gy)
        dx = torch.empty_like(y)
        call("stts_leaky_relu_bwd", y, dy, y.numel(), ctx.slope, dx)
        return dx, None


def leaky_relu(x, slope):
    return _LReLUFn.apply(x, float(slope))


class _WNConv2dK1(nn.Module):
    """weight_norm(nn.Conv2d(cin, cout, (k, 1), (stride, 1), padding=(pad, 0))) parameter layout."""

    def __init__(self, cin, cout, k, stride, pad):
        super().__init__()
        self.weight_g = nn.Parameter(torch.ones(cout, 1, 1, 1))
        self.weight_v = nn.Parameter(torch.randn(cout, cin, k, 1) * 0.05)
        self.bias = nn.Parameter(torch.zeros(cout))
        self.k, self.stride, self.pad = k, stride, pad


class DiscriminatorP(nn.Module):
    """Trainable Modules/discriminators.py:96-129 DiscriminatorP (weight-norm, k 5, stride 3; same
    parameter names), forward and backward on the HIP kernels.  Each (k, 1) Conv2d is a conv1d along
    the H axis of every one of the `period` columns: the [B, C, H, p] map is kept as frames
    [B * p, H, C] between layers.  forward(x [B, 1, T]) -> (score [B, H * p], fmap [B, C, H, p] x 6)
    as the reference."""

    def __init__(self, period, kernel_size=5, stride=3, dtype_compute="fp32"):
        super().__init__()
        self.period = period
        self.dtype_compute = dtype_compute  # 'bf16': bf16 operands for the conv forwards and dx
        ch = [1, 32, 128, 512, 1024, 1024]
        self.convs = nn.ModuleList([_WNConv2dK1(ch[j], ch[j + 1], kernel_size, stride if j < 4 else 1, 2)
                                    for j in range(5)])
        self.conv_post = _WNConv2dK1(1024, 1, 3, 1, 1)

    def forward(self, x):
        b, c, t = x.shape
        p = self.period
        if t % p != 0:
            x = torch.nn.functional.pad(x, (0, p - t % p), "reflect")  # discriminators.py:112-115
            t = x.shape[-1]
        h = x.reshape(b, c, t // p, p).permute(0, 3, 2, 1).reshape(b * p, t // p, c)  # frames [B p, H, C]
        fmap = []

        def nchw(f):
            return f.reshape(b, p, f.shape[1], f.shape[2]).permute(0, 3, 2, 1)

        for layer in self.convs:
            w = weight_norm(layer.weight_g, layer.weight_v)
            h = conv1d_frames(h, w.reshape(w.shape[0], w.shape[1], layer.k), layer.bias, layer.stride, layer.pad,
                              dtype=self.dtype_compute)
            h = leaky_relu(h, 0.1)
            fmap.append(nchw(h))
        cp = self.conv_post
        w = weight_norm(cp.weight_g, cp.weight_v)
        h = conv1d_frames(h, w.reshape(1, w.shape[1], cp.k), cp.bias, 1, cp.pad, dtype=self.dtype_compute)
        out = nchw(h)
        fmap.append(out)
        return torch.flatten(out, 1, -1), fmap


# ====================================================================== the assembled training step (config 5)
# train.py:267-327: the decoder forward (Modules/hifigan.py:446-475) with its parameters' gradients, the
# discriminators (Modules/discriminators.py) with theirs, the losses (losses.py) and AdamW (optimizers.py).
# Every Function below runs its forward and backward as HIP kernels (include/stts2_train.h).

class _SnakeFn(torch.autograd.Function):
    """Snake with a learned alpha (the Generator's stage activations, hifigan.py:329, :343) on frames."""

    @staticmethod
    def forward(ctx, x, alpha):
        _require_device()
        B, L, C = x.shape
        xc, ac = _c(x), _c(alpha.reshape(-1))
        y = torch.empty_like(xc)
        call("stts_snake_fwd", xc, ac, B, L, C, y)
        ctx.save_for_backward(xc, ac)
        ctx.a_shape = alpha.shape
        return y

    @staticmethod
    def backward(ctx, dy):
        xc, ac = ctx.saved_tensors
        B, L, C = xc.shape
        nx, na = ctx.needs_input_grad
        dyc = _c(dy)
        dx = torch.empty_like(xc) if nx else None
        da = torch.empty(C, dtype=torch.float32, device=dyc.device) if na else None
        call("stts_snake_bwd", xc, ac, dyc, B, L, C, dx, da, ws=("stts_snake_workspace_bytes", B, L, C))
        return dx, (da.reshape(ctx.a_shape) if da is not None else None)


def snake(x, alpha):
    return _SnakeFn.apply(x, alpha)


class _TanhFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        _require_device()
        xc = _c(x)
        y = torch.empty_like(xc)
        call("stts_tanh_fwd", xc, xc.numel(), y)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dyc = _c(dy)
        dx = torch.empty_like(y)
        call("stts_tanh_bwd", y, dyc, y.numel(), dx)
        return dx


def tanh(x):
    return _TanhFn.apply(x)


class _SumDivFn(torch.autograd.Function):
    """(x0 + x1 + ...) / div, added left to right (x + x_source, hifigan.py:334; xs / num_kernels, :342)."""

    @staticmethod
    def forward(ctx, div, *xs):
        _require_device()
        xc = [_c(x) for x in xs]
        for x in xc[1:]:
            if x.shape != xc[0].shape:
                raise ValueError(f"sum of tensors of shapes {[tuple(t.shape) for t in xc]}")
        y = torch.empty_like(xc[0])
        arr = (ctypes.c_void_p * len(xc))(*[x.data_ptr() for x in xc])
        call("stts_sum_div", arr, len(xc), y.numel(), div, y)
        ctx.div, ctx.n = float(div), len(xc)
        return y

    @staticmethod
    def backward(ctx, dy):
        if ctx.div == 1.0:
            g = dy
        else:
            dyc = _c(dy)
            g = torch.empty_like(dyc)
            call("stts_div", dyc, dyc.numel(), ctx.div, g)
        # every input gets its own tensor: the inputs may come from concurrent branches (CONCURRENT_BRANCHES), and
        # autograd may accumulate a gradient in place on one stream while another branch's stream still reads a
        # shared one
        out, first = [], True
        for need in ctx.needs_input_grad[1:]:
            out.append((g if first else g.clone()) if need else None)
            first = first and not need
        return (None,) + tuple(out)


def sum_div(xs, div=1.0):
    return _SumDivFn.apply(float(div), *xs)


class _SourceFn(torch.autograd.Function):
    """SourceModuleHnNSF (hifigan.py:221-268): f0_curve [B, n] -> har [B, n*scale]; gradients for l_linear."""

    @staticmethod
    def forward(ctx, f0_curve, lw, lb, noise, seed, utt_offset, scale):
        _require_device()
        B, n = f0_curve.shape
        L = n * scale
        fc, wc, bc = _c(f0_curve), _c(lw.reshape(-1)), _c(lb.reshape(-1))
        nz = _c(noise)
        if nz is not None and tuple(nz.shape) != (B, L, 9):
            raise ValueError(f"noise {tuple(nz.shape)}: expected {(B, L, 9)}")
        sw = torch.empty(B, L, 9, dtype=torch.float32, device=fc.device)
        har = torch.empty(B, L, dtype=torch.float32, device=fc.device)
        ws = ("stts_source_workspace_bytes", B, n)
        if isinstance(seed, torch.Tensor):  # a device int64 [1] (the capturable step): the kernel reads it
            if not seed.is_cuda or seed.dtype != torch.int64:
                raise TypeError("seed tensor: int64 on the device")
            call("stts_source_fwd_seed_dev", fc, wc, bc, nz, seed, int(utt_offset), B, n, int(scale), sw, har, ws=ws)
        else:
            call("stts_source_fwd", fc, wc, bc, nz, ctypes.c_ulonglong(int(seed) & (2**64 - 1)), int(utt_offset), B, n,
                 int(scale), sw, har, ws=ws)
        ctx.save_for_backward(sw, har)
        ctx.shapes = (lw.shape, lb.shape, n)
        return har

    @staticmethod
    def backward(ctx, dhar):
        sw, har = ctx.saved_tensors
        lw_shape, lb_shape, n = ctx.shapes
        B, L = har.shape
        nw, nbias = ctx.needs_input_grad[1:3]
        if not (nw or nbias):
            return (None,) * 7
        d = _c(dhar)
        dW = torch.empty(9, dtype=torch.float32, device=d.device)
        db = torch.empty(1, dtype=torch.float32, device=d.device)
        call("stts_source_bwd", sw, har, d, B, L, dW, db, ws=("stts_source_workspace_bytes", B, n))
        return None, (dW.reshape(lw_shape) if nw else None), (db.reshape(lb_shape) if nbias else None), None, None, \
            None, None


class _BoxFn(torch.autograd.Function):
    """conv1d(x, ones(1, 1, k), padding k // 2) / k per row (the train-mode smoothing, hifigan.py:453-455)."""

    @staticmethod
    def forward(ctx, x, k):
        _require_device()
        xc = _c(x)
        B, n = xc.shape
        y = torch.empty_like(xc)
        call("stts_box_smooth_fwd", xc, B, n, int(k), y)
        ctx.k = int(k)
        return y

    @staticmethod
    def backward(ctx, dy):
        d = _c(dy)
        B, n = d.shape
        dx = torch.empty_like(d)
        call("stts_box_smooth_bwd", d, B, n, ctx.k, dx)
        return dx, None


def box_smooth(x, k):
    return _BoxFn.apply(x, int(k))


def train_smooth(F0_curve, N, rng=None):
    """Decoder.forward's train-mode branch (hifigan.py:447-455): F0_down from [0, 3, 7] and N_down from
    [0, 3, 7, 15], drawn with Python's `random.randint` in the reference's order (so random.seed governs
    them), then the box smoothing on the device."""
    import random as _random
    r = rng or _random
    F0_down = [0, 3, 7][r.randint(0, 2)]
    N_down = [0, 3, 7, 15][r.randint(0, 3)]
    if F0_down:
        F0_curve = box_smooth(F0_curve, F0_down)
    if N_down:
        N = box_smooth(N, N_down)
    return F0_curve, N


class _TimeExpandFn(torch.autograd.Function):
    """x3[s][h][w][c*3 + dh] = y[s][h + dh - 1][w][c]: a (3, kw) Conv2d as a 1-D conv over 3C channels."""

    @staticmethod
    def forward(ctx, y):
        _require_device()
        yc = _c(y)
        S, H, W, C = yc.shape
        x3 = torch.empty(S, H, W, 3 * C, dtype=torch.float32, device=yc.device)
        call("stts_time_expand3", yc, S, H, W, C, x3)
        ctx.shape = (S, H, W, C)
        return x3

    @staticmethod
    def backward(ctx, dx3):
        S, H, W, C = ctx.shape
        d = _c(dx3)
        dy = torch.empty(S, H, W, C, dtype=torch.float32, device=d.device)
        call("stts_time_expand3_bwd", d, S, H, W, C, dy)
        return dy


# the MSD's (3, kw) Conv2d over C = 32 channels as one launch that time-expands in its window loads
# (stts_conv1d_fwd_tx); False = the materialised x3 + conv1d_frames (tests compare both)
FUSE_TX = True
# (K, stride) of the MSD layers whose bf16 weight gradient reads the image directly (stts_conv1d_wgrad_tx)
_WGRAD_TX = {(3, 1), (9, 2)}


class _ConvTxFn(torch.autograd.Function):
    """SpecDiscriminator's Conv2d(C, Cout, (3, kw), stride (1, s), padding (1, pad)) + optional leaky ReLU on the
    image h [S, H, W, C] -> frames [S H, Lq, Cout], with the time expansion inside the conv (stts_conv1d_fwd_tx,
    weight permuted to dh-major).  Backward: d h by stts_conv1d_bwd_tx (Cout = 32: dy expanded by the engine's
    loads, weight rows reversed) or, for the Cout = 1 out layer, stts_conv1d_bwd on x3 + stts_time_expand3_bwd;
    d w / d b by stts_conv1d_bwd over the materialised x3 (c-major, the weight as it lies)."""

    @staticmethod
    def forward(ctx, h, w, bias, stride, pad, dtype, act):
        _require_device()
        hf = _c(h)
        S, H, W, C = hf.shape
        co, ci, kh, kw = w.shape
        if ci != C or kh != 3:
            raise ValueError(f"weight {tuple(w.shape)} does not take the [S, H, W, {C}] image")
        Lq = out_length(W, kw, stride, pad, 1)
        dt = _DT[dtype]
        wc = _c(w)
        wtx = wc.permute(0, 2, 1, 3).contiguous()  # [Cout][3][C][kw]: K index dh C + c
        bc = _c(bias)
        y = torch.empty(S * H, Lq, co, dtype=torch.float32, device=hf.device)
        call("stts_conv1d_fwd_tx", dt, hf, wtx, bc, S, H, W, C, co, kw, stride, pad, Lq, int(act is not None),
             act if act is not None else 0.0, y,
             ws=("stts_conv1d_fwd_tx_workspace_bytes", dt, S, H, W, C, co, kw, stride, pad, Lq))
        ctx.save_for_backward(hf, wc, y if act is not None else None)
        ctx.geo = (S, H, W, C, co, kw, stride, pad, Lq, dt, bias is not None)
        ctx.act = act
        _count("fwd", 2.0 * S * H * Lq * co * 3 * C * kw)
        return y

    @staticmethod
    def backward(ctx, gy):
        hf, wc, ya = ctx.saved_tensors
        S, H, W, C, co, kw, stride, pad, Lq, dt, has_bias = ctx.geo
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        dyf = _c(gy)
        if ctx.act is not None:
            dpre = torch.empty_like(dyf)
            call("stts_leaky_relu_bwd", ya, dyf, ya.numel(), ctx.act, dpre)
            dyf = dpre
        dev = dyf.device
        B, Cin = S * H, 3 * C
        dh = None
        if need_x and co == 32:  # d h straight from dy (no dx3 image, no fold)
            wd = wc.flip(2).permute(2, 0, 1, 3).contiguous()  # [3][Cout][C][kw]: chunk j = row dh = 2 - j
            dh = torch.empty(S, H, W, C, dtype=torch.float32, device=dev)
            call("stts_conv1d_bwd_tx", dt, dyf, wd, S, H, W, C, co, kw, stride, pad, Lq, dh,
                 ws=("stts_conv1d_bwd_tx_workspace_bytes", dt, S, H, W, C, co, kw, stride, pad, Lq))
            _count("bwd", 2.0 * B * Lq * co * Cin * kw)
            need_x = False
        need_b = need_b and has_bias
        dx3 = dw = db = None
        if not need_x and (need_w or need_b) and dt == 1 and (kw, stride) in _WGRAD_TX:  # bf16: no x3 either
            dwt = torch.empty(co, 3, C, kw, dtype=torch.float32, device=dev)
            db = torch.empty(co, dtype=torch.float32, device=dev) if need_b else None
            call("stts_conv1d_wgrad_tx", dt, hf, dyf, S, H, W, C, co, kw, stride, pad, Lq, dwt, db,
                 ws=("stts_conv1d_bwd_workspace_bytes", dt, B, W, Cin, co, kw, stride, 1, pad, Lq))
            _count("bwd", 2.0 * B * Lq * co * Cin * kw)
            dw = dwt.permute(0, 2, 1, 3) if need_w else None  # -> [Cout][C][3][kw]
            need_w = need_b = False
        if need_x or need_w or need_b:  # (the G step's frozen discriminators skip this: d h only)
            x3 = torch.empty(S, H, W, Cin, dtype=torch.float32, device=dev)
            call("stts_time_expand3", hf, S, H, W, C, x3)
            dx3 = torch.empty(B, W, Cin, dtype=torch.float32, device=dev) if need_x else None
            dw = torch.empty(co, Cin, kw, dtype=torch.float32, device=dev) if need_w else None
            db = torch.empty(co, dtype=torch.float32, device=dev) if need_b else None
            call("stts_conv1d_bwd", dt, x3, wc, dyf, B, W, Cin, co, kw, stride, 1, pad, Lq, dx3, dw, db,
                 ws=("stts_conv1d_bwd_workspace_bytes", dt, B, W, Cin, co, kw, stride, 1, pad, Lq))
            _count("bwd", 2.0 * B * Lq * co * Cin * kw * ((dx3 is not None) + (dw is not None)))
        if dx3 is not None:
            dh = torch.empty(S, H, W, C, dtype=torch.float32, device=dev)
            call("stts_time_expand3_bwd", dx3, S, H, W, C, dh)
        if dw is not None and dw.dim() == 3:
            dw = dw.reshape(co, C, 3, kw)
        return dh, dw, db, None, None, None, None


class _StftMagFn(torch.autograd.Function):
    """|torch.stft(x, n_fft, hop, win, hann(win))| (discriminators.py:11-27) as the [S, F, nb] image."""

    @staticmethod
    def forward(ctx, wave, n_fft, hop, win):
        _require_device()
        w = _c(wave)
        S, L = w.shape
        F_ = 1 + L // hop
        nb = n_fft // 2 + 1
        mag = torch.empty(S, F_, nb, dtype=torch.float32, device=w.device)
        spec = torch.empty(S, F_, nb, 2, dtype=torch.float32, device=w.device)
        call("stts_stft_mag_fwd", w, S, L, L, n_fft, win, hop, mag, spec)
        ctx.save_for_backward(spec)
        ctx.geo = (S, L, n_fft, win, hop)
        return mag

    @staticmethod
    def backward(ctx, dmag):
        (spec,) = ctx.saved_tensors
        S, L, n_fft, win, hop = ctx.geo
        d = _c(dmag)
        dw = torch.empty(S, L, dtype=torch.float32, device=d.device)
        call("stts_stft_mag_bwd", spec, d, S, L, n_fft, win, hop, dw,
             ws=("stts_stft_mag_workspace_bytes", S, L, n_fft, win, hop))
        return dw, None, None, None


def stft_mag(wave, n_fft, hop, win):
    return _StftMagFn.apply(wave, int(n_fft), int(hop), int(win))


# ---------------------------------------------------------------------- decoder (Modules/hifigan.py)
def _wn_w(layer):
    """The folded weight of a weight-normed layer in either layout: torch.nn.utils.weight_norm's weight_g / weight_v
    (hifigan.py) or parametrizations.weight_norm's parametrizations.weight.original0 (g) / original1 (v) (vocos.py:10)."""
    if hasattr(layer, "parametrizations"):
        p = layer.parametrizations["weight"]
        return weight_norm(p.original0, p.original1)
    return weight_norm(layer.weight_g, layer.weight_v)


# independent branches of the generator (the noise branch beside snake -> ups, the num_kernels resblocks of a
# stage) run on their own HIP streams, as discriminators.CONCURRENT does for the sub-discriminators; autograd runs
# each backward op on its forward's stream.  False = one stream (A/B, tests)
CONCURRENT_BRANCHES = True
_BRANCH_STREAMS = {}


def _branches(fns, inputs=()):
    """[f() for f in fns], f i on side stream i, ordered after the caller's stream, which waits for all of them;
    `inputs` (tensors of the caller's stream the branches read or save for backward) are recorded on each side
    stream so the allocator does not hand their memory out before those reads finish."""
    if not CONCURRENT_BRANCHES or len(fns) < 2:
        return [f() for f in fns]
    dev = torch.device("cuda", torch.cuda.current_device())
    key = (dev.index, len(fns))
    if key not in _BRANCH_STREAMS:
        _BRANCH_STREAMS[key] = [torch.cuda.Stream(device=dev) for _ in fns]
    main = torch.cuda.current_stream(dev)
    outs = []
    for f, st in zip(fns, _BRANCH_STREAMS[key]):
        st.wait_stream(main)
        for t in inputs:
            t.record_stream(st)
        with torch.cuda.stream(st):
            outs.append(f())
    for st in _BRANCH_STREAMS[key]:
        main.wait_stream(st)
    for o in outs:
        o.record_stream(main)
    return outs


def generator_forward(g, x, s, f0_curve, noise=None, seed=0, utt_offset=0, dtype="fp32"):
    """Generator.forward (hifigan.py:321-347) on frames x [B, 2T, 512] for a module with the reference's
    parameter layout (stts2_mi355x.hifigan.Generator) -> waveform frames [B, L, 1]."""
    rates, kernels = g.upsample_rates, g.upsample_kernel_sizes
    nk = g.num_kernels
    scale = int(g.upsample_scale)
    har = _SourceFn.apply(f0_curve, g.m_source.l_linear.weight, g.m_source.l_linear.bias, noise, seed, utt_offset,
                          scale).unsqueeze(-1)  # frames [B, L, 1]
    B = har.shape[0]
    for i, (u, k) in enumerate(zip(rates, kernels)):
        nc = g.noise_convs[i]

        def noise_branch(i=i, nc=nc):
            S, P = int(nc.stride), int(nc.padding)
            if S > 1 and nc.weight.shape[-1] == 2 * S and 2 * P == S:
                # Conv1d(1, C, 2S, stride S, padding S/2) (hifigan.py:296-299) as a 2-tap stride-1 conv over
                # S-sample frames: frame r = samples [r S - P, r S - P + S), w'[c][j][t] = w[c][0][t S + j]
                fr = torch.nn.functional.pad(har[..., 0], (P, S - P)).reshape(B, -1, S)
                w2 = nc.weight.reshape(nc.weight.shape[0], 2, S).transpose(1, 2)
                x_src = conv1d_frames(fr, w2, nc.bias, 1, 0, 1, dtype)
            else:
                x_src = conv1d_frames(har, nc.weight, nc.bias, nc.stride, nc.padding, 1, dtype)
            return resblock1_frames(g.noise_res[i], x_src, s, dtype)

        def up_branch(i=i, x=x):
            x = snake(x, g.alphas[i])
            up = g.ups[i]
            return conv_transpose1d_frames(x, _wn_w(up), up.bias, up.stride, up.padding, up.output_padding, dtype)

        x, x_src = _branches([up_branch, noise_branch], (x, har, s))
        x = sum_div([x, x_src])
        rs = _branches([lambda j=j, x=x: resblock1_frames(g.resblocks[i * nk + j], x, s, dtype) for j in range(nk)],
                       (x, s))
        x = sum_div(rs, nk)
    x = snake(x, g.alphas[len(rates)])
    cp = g.conv_post
    x = conv1d_frames(x, _wn_w(cp), cp.bias, 1, cp.padding, 1, dtype)
    return tanh(x)


def decoder_forward(dec, asr, F0_curve, N, s, noise=None, seed=None, utt_offset=0, dtype="fp32"):
    """Decoder.forward (hifigan.py:446-475) with autograd through HIP kernels: asr [B, 512, T], F0_curve and
    N [B, 2T], s [B, style_dim] -> [B, 1, 600 T].  `dec` is stts2_mi355x.hifigan.Decoder (reference
    parameter names); in .train() mode the F0 / N smoothing of :447-455 is applied first (Python's random,
    as the reference).  Activations stay in frames [B, L, C] end to end."""
    _require_device()
    if dtype not in _DT:
        raise ValueError(f"dtype {dtype!r}: expected one of {list(_DT)}")
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if noise is None else 0
    if dec.training:
        F0_curve, N = train_smooth(F0_curve, N)
    B = asr.shape[0]
    x = _decoder_frontend(dec, asr, F0_curve, N, s, dtype)
    y = generator_forward(dec.generator, x, s, F0_curve, noise, seed, utt_offset, dtype)  # [B, L, 1]
    return y.reshape(B, 1, -1)


def _decoder_frontend(dec, asr, F0_curve, N, s, dtype, kchunk=0):
    """The front-end the three decoders share (hifigan.py:458-472 == vocos.py:404-418): the stride-2 F0 / N convs,
    encode, asr_res and the decode blocks with their concats -> frames [B, 2T, 512].  Reads either weight-norm
    layout (_wn_w)."""
    T = asr.shape[2]
    if F0_curve.shape[-1] != 2 * T or N.shape[-1] != 2 * T:
        raise ValueError(f"F0_curve / N {tuple(F0_curve.shape)} / {tuple(N.shape)}: expected [B, {2 * T}]")
    F0 = conv1d_frames(F0_curve.unsqueeze(-1), _wn_w(dec.F0_conv), dec.F0_conv.bias, 2, 1, 1, dtype)  # [B, T, 1]
    Nc = conv1d_frames(N.unsqueeze(-1), _wn_w(dec.N_conv), dec.N_conv.bias, 2, 1, 1, dtype)
    asr_f = asr.transpose(1, 2)  # frames [B, T, 512]
    x = torch.cat([asr_f, F0, Nc], dim=2)
    x = adain_resblk1d_frames(dec.encode, x, s, dtype, kchunk)
    ar = dec.asr_res[0]
    asr_res = conv1d_frames(asr_f, _wn_w(ar), ar.bias, 1, 0, 1, dtype)
    res = True
    for block in dec.decode:
        if res:
            x = torch.cat([x, asr_res, F0, Nc], dim=2)
        x = adain_resblk1d_frames(block, x, s, dtype, kchunk)
        if block.upsample_type != "none":
            res = False
    return x


# ---------------------------------------------------------------------- Vocos decoder (Modules/vocos.py)
class _DWConvFn(torch.autograd.Function):
    """ConvNeXtBlock.dwconv (vocos.py:45): depthwise Conv1d(C, C, K, padding K // 2) on frames [B, L, C]; w [C, 1, K]."""

    @staticmethod
    def forward(ctx, x, w, bias):
        _require_device()
        B, L, C = x.shape
        K = w.shape[-1]
        xc, wc, bc = _c(x), _c(w).reshape(C, K), _c(bias)
        y = torch.empty_like(xc)
        call("stts_dwconv1d_fwd", xc, wc, bc, B, L, C, K, y)
        ctx.save_for_backward(xc, wc)
        ctx.w_shape, ctx.has_b = w.shape, bias is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        xc, wc = ctx.saved_tensors
        B, L, C = xc.shape
        K = wc.shape[1]
        dy = _c(gy)
        nx, nw, nbias = ctx.needs_input_grad
        dx = torch.empty_like(xc) if nx else None
        dw = torch.empty(C, K, dtype=torch.float32, device=dy.device) if nw else None
        db = torch.empty(C, dtype=torch.float32, device=dy.device) if (nbias and ctx.has_b) else None
        call("stts_dwconv1d_bwd", xc, wc, dy, B, L, C, K, dx, dw, db,
             ws=("stts_dwconv1d_bwd_workspace_bytes", B, L, C, K))
        return dx, (dw.reshape(ctx.w_shape) if dw is not None else None), db


def dwconv1d_frames(x, weight, bias=None):
    return _DWConvFn.apply(x, weight, bias)


class _GeluFn(torch.autograd.Function):
    """nn.GELU() (erf form, vocos.py:48); the backward reads the saved pre-activation."""

    @staticmethod
    def forward(ctx, x):
        _require_device()
        xc = _c(x)
        y = torch.empty_like(xc)
        call("stts_gelu_fwd", xc, xc.numel(), y)
        ctx.save_for_backward(xc)
        return y

    @staticmethod
    def backward(ctx, gy):
        (xc,) = ctx.saved_tensors
        dy = _c(gy)
        dx = torch.empty_like(xc)
        call("stts_gelu_bwd", xc, dy, xc.numel(), dx)
        return dx


def gelu(x):
    return _GeluFn.apply(x)


class _LayerScaleResFn(torch.autograd.Function):
    """y = r + gamma x on frames [B, L, C] (vocos.py:64-68); the residual's gradient is dy itself."""

    @staticmethod
    def forward(ctx, x, r, gamma):
        _require_device()
        B, L, C = x.shape
        xc, rc, gc = _c(x), _c(r), _c(gamma)
        if rc.shape != xc.shape or gc.numel() != C:
            raise ValueError(f"layer scale: x {tuple(x.shape)}, r {tuple(r.shape)}, gamma {tuple(gamma.shape)}")
        y = torch.empty_like(xc)
        call("stts_layer_scale_res_fwd", xc, rc, gc, B, L, C, y)
        ctx.save_for_backward(xc, gc)
        ctx.g_shape = gamma.shape
        return y

    @staticmethod
    def backward(ctx, gy):
        xc, gc = ctx.saved_tensors
        B, L, C = xc.shape
        dy = _c(gy)
        nx, nr, ng = ctx.needs_input_grad
        dx = torch.empty_like(xc) if nx else None
        dg = torch.empty(C, dtype=torch.float32, device=dy.device) if ng else None
        call("stts_layer_scale_res_bwd", xc, gc, dy, B, L, C, dx, dg,
             ws=("stts_layer_scale_res_bwd_workspace_bytes", B, L, C))
        return dx, (gy if nr else None), (dg.reshape(ctx.g_shape) if dg is not None else None)


def layer_scale_res(x, r, gamma):
    return _LayerScaleResFn.apply(x, r, gamma)


class _ISTFTHeadFn(torch.autograd.Function):
    """ISTFTHead after its Linear + ISTFT 'same' (vocos.py:282-296, :190-232): h [B, F, n_fft + 2] -> audio [B, F hop].
    The window is a buffer (no gradient)."""

    @staticmethod
    def forward(ctx, h, window, n_fft, hop):
        _require_device()
        B, F, W = h.shape
        if W != n_fft + 2 or window.numel() != n_fft:
            raise ValueError(f"ISTFT head: h {tuple(h.shape)}, window {tuple(window.shape)} for n_fft {n_fft}")
        hc, wc = _c(h), _c(window)
        y = torch.empty(B, F * hop, dtype=torch.float32, device=h.device)
        call("stts_istft_head_fwd", hc, wc, B, F, n_fft, hop, y, ws=("stts_istft_head_workspace_bytes", B, F, n_fft, hop))
        ctx.save_for_backward(hc, wc)
        ctx.geo = (n_fft, hop)
        return y

    @staticmethod
    def backward(ctx, gy):
        hc, wc = ctx.saved_tensors
        n_fft, hop = ctx.geo
        B, F, _ = hc.shape
        dy = _c(gy)
        dh = torch.empty_like(hc)
        call("stts_istft_head_bwd", hc, wc, dy, B, F, n_fft, hop, dh, None, 0)
        return dh, None, None, None


def istft_head(h, window, n_fft, hop):
    return _ISTFTHeadFn.apply(h, window, int(n_fft), int(hop))


def convnext_block_frames(m, x, s, dtype="fp32"):
    """ConvNeXtBlock.forward (vocos.py:56-69) on frames x [B, L, C] for a module with the reference's parameter
    layout (stts2_mi355x.vocos.ConvNeXtBlock): dwconv -> AdaIN1d -> pwconv1 -> GELU -> pwconv2 -> x + gamma * (.)."""
    h = dwconv1d_frames(x, m.dwconv.weight, m.dwconv.bias)
    h = adain_act(h, s, m.norm.fc.weight, m.norm.fc.bias, None, ACT_NONE)
    h = conv1d_frames(h, m.pwconv1.weight.unsqueeze(-1), m.pwconv1.bias, dtype=dtype)  # nn.Linear as [N][K][1]
    h = gelu(h)
    h = conv1d_frames(h, m.pwconv2.weight.unsqueeze(-1), m.pwconv2.bias, dtype=dtype)
    return layer_scale_res(h, x, m.gamma)


def vocos_generator_forward(g, x, s, dtype="fp32"):
    """Generator.forward (vocos.py:157-162) + ISTFTHead.forward (:271-296) on frames x [B, F, dim] -> [B, F hop]."""
    from .texttrain import layer_norm_act  # stts_row_norm / stts_row_norm_bwd, mode 0 (texttrain imports this module)
    for blk in g.convnext:
        x = convnext_block_frames(blk, x, s, dtype)
    ln = g.final_layer_norm
    x = layer_norm_act(x, ln.weight, ln.bias, ln.eps, None, None)  # eps 1e-6, no LeakyReLU, no row mask
    head = g.stft
    n_fft, hop = int(head.n_fft), int(head.hop_length)
    W, b = head.out.weight, head.out.bias
    # the head Linear has n_fft + 2 output columns (1202 / 1026): zero weight rows pad them to the conv engines'
    # 16-column multiple and the output is sliced, so autograd returns the gradients of the real rows
    padn = -W.shape[0] % 16
    if padn:
        W = torch.cat([W, W.new_zeros(padn, W.shape[1])])
        b = torch.cat([b, b.new_zeros(padn)])
    h = conv1d_frames(x, W.unsqueeze(-1), b, dtype=dtype)[..., :n_fft + 2]
    return istft_head(h, head.istft.window, n_fft, hop)


def vocos_decoder_forward(dec, asr, F0_curve, N, s, dtype="fp32"):
    """Decoder.forward (vocos.py:392-421) with autograd through HIP kernels: asr [B, 512, T], F0_curve and N [B, 2T],
    s [B, style_dim] -> [B, 1, 2T hop].  `dec` is stts2_mi355x.vocos.Decoder; in .train() mode the F0 / N smoothing
    of :393-401 is applied first (Python's random, as the reference).  The convs and GEMMs take `dtype` (fp32, bf16,
    bf16x3) as for HiFi-GAN; the depthwise conv, GELU, layer scale and ISTFT head are fp32 frames in all three."""
    _require_device()
    if dtype not in _DT:
        raise ValueError(f"dtype {dtype!r}: expected one of {list(_DT)}")
    if dec.training:
        F0_curve, N = train_smooth(F0_curve, N)
    x = _decoder_frontend(dec, asr, F0_curve, N, s, dtype)
    return vocos_generator_forward(dec.generator, x, s, dtype).unsqueeze(1)


# ---------------------------------------------------------------------- iSTFTNet decoder (Modules/istftnet.py)
FRONT_KCHUNK = 512  # channel block of the fp32 front-end convs of istft_decoder_forward (0 = one chain per output)
class _CSTFTFn(torch.autograd.Function):
    """CustomSTFT.transform (istftnet.py:207-243): wave [B, L] -> frames [B, L // hop + 1, n_fft + 2] (magnitude
    channels, then phase).  The reference computes it under no_grad (:544-550): the output is a constant."""

    @staticmethod
    def forward(ctx, wave, wr, wi, n_fft, hop):
        _require_device()
        w = _c(wave)
        B, L = w.shape
        nb = n_fft // 2 + 1
        if wr.numel() != nb * n_fft or wi.numel() != nb * n_fft:
            raise ValueError(f"CustomSTFT: forward bases {tuple(wr.shape)} / {tuple(wi.shape)} for n_fft {n_fft}")
        out = torch.empty(B, L // hop + 1, n_fft + 2, dtype=torch.float32, device=w.device)
        call("stts_cstft_fwd", w, _c(wr), _c(wi), B, L, n_fft, hop, out)
        ctx.mark_non_differentiable(out)
        return out

    @staticmethod
    def backward(ctx, g):
        return None, None, None, None, None


def cstft(wave, wr, wi, n_fft, hop):
    return _CSTFTFn.apply(wave, wr, wi, int(n_fft), int(hop))


class _PadLAddFn(torch.autograd.Function):
    """reflection_pad((1, 0))(x) + src on frames (istftnet.py:558-561): x [B, L, C], src [B, L + 1, C]."""

    @staticmethod
    def forward(ctx, x, src):
        _require_device()
        B, L, C = x.shape
        if tuple(src.shape) != (B, L + 1, C):
            raise ValueError(f"padl_add: x {tuple(x.shape)}, src {tuple(src.shape)}: expected {(B, L + 1, C)}")
        xc, sc = _c(x), _c(src)
        y = torch.empty_like(sc)
        call("stts_padl_add_fwd", xc, sc, B, L, C, y)
        ctx.shape = (B, L, C)
        return y

    @staticmethod
    def backward(ctx, gy):
        B, L, C = ctx.shape
        nx, ns = ctx.needs_input_grad
        dx = None
        if nx:
            dy = _c(gy)
            dx = torch.empty(B, L, C, dtype=torch.float32, device=dy.device)
            call("stts_padl_add_bwd", dy, B, L, C, dx)
        return dx, (gy if ns else None)  # dx is its own tensor (see _SumDivFn.backward); src's gradient is dy itself


def padl_add(x, src):
    return _PadLAddFn.apply(x, src)


class _CISTFTHeadFn(torch.autograd.Function):
    """exp / sin -> CustomSTFT.inverse (istftnet.py:571-573, :246-293): post [B, F, n_fft + 2] -> audio
    [B, (F - 1) hop].  Only `post` is saved; the bases are buffers (no gradient)."""

    @staticmethod
    def forward(ctx, post, br, bi, n_fft, hop):
        _require_device()
        B, F, W = post.shape
        nb = n_fft // 2 + 1
        if W != 2 * nb or br.numel() != nb * n_fft or bi.numel() != nb * n_fft:
            raise ValueError(f"CustomSTFT head: post {tuple(post.shape)}, bases {tuple(br.shape)} / {tuple(bi.shape)} "
                             f"for n_fft {n_fft}")
        pc, brc, bic = _c(post), _c(br), _c(bi)
        y = torch.empty(B, max(F - 1, 0) * hop, dtype=torch.float32, device=pc.device)
        call("stts_cistft_head_fwd", pc, brc, bic, B, F, n_fft, hop, y)
        ctx.save_for_backward(pc, brc, bic)
        ctx.geo = (n_fft, hop)
        return y

    @staticmethod
    def backward(ctx, gy):
        pc, brc, bic = ctx.saved_tensors
        n_fft, hop = ctx.geo
        B, F, _ = pc.shape
        dy = _c(gy)
        dp = torch.empty_like(pc)
        call("stts_cistft_head_bwd", pc, brc, bic, dy, B, F, n_fft, hop, dp)
        return dp, None, None, None, None


def cistft_head(post, br, bi, n_fft, hop):
    return _CISTFTHeadFn.apply(post, br, bi, int(n_fft), int(hop))


def istft_generator_forward(g, x, s, f0_curve, noise=None, seed=0, utt_offset=0, dtype="fp32"):
    """Generator.forward (istftnet.py:543-573) on frames x [B, 2T, 512] for a module with the reference's parameter
    layout (stts2_mi355x.istftnet.Generator) -> audio [B, 2T prod(rates) hop].  The harmonic source and its STFT
    are constants, as under the reference's no_grad (:544-550): m_source.l_linear receives no gradient and
    f0_curve's gradient comes through the front-end's F0_conv only."""
    rates, kernels = g.upsample_rates, g.upsample_kernel_sizes
    nk, last = g.num_kernels, len(rates) - 1
    n_fft, hop = int(g.gen_istft_n_fft), int(g.gen_istft_hop_size)
    st = g.stft
    with torch.no_grad():
        lin = g.m_source.l_linear
        src = _SourceFn.apply(f0_curve.detach(), lin.weight.detach(), lin.bias.detach(), noise, seed, utt_offset,
                              int(g.upsample_scale))  # [B, L], L = 2T prod(rates) hop
        har = cstft(src, st.weight_forward_real, st.weight_forward_imag, n_fft, hop)  # frames [B, L / hop + 1, n_fft + 2]
    for i, (u, k) in enumerate(zip(rates, kernels)):
        nc = g.noise_convs[i]

        def noise_branch(i=i, nc=nc):
            x_src = conv1d_frames(har, nc.weight, nc.bias, int(nc.stride), int(nc.padding), 1, dtype)
            return resblock1_frames(g.noise_res[i], x_src, s, dtype)

        def up_branch(i=i, x=x):
            x = leaky_relu(x, 0.1)
            up = g.ups[i]
            return conv_transpose1d_frames(x, _wn_w(up), up.bias, up.stride, up.padding, up.output_padding, dtype)

        x, x_src = _branches([up_branch, noise_branch], (x, har, s))
        x = padl_add(x, x_src) if i == last else sum_div([x, x_src])
        rs = _branches([lambda j=j, x=x: resblock1_frames(g.resblocks[i * nk + j], x, s, dtype) for j in range(nk)],
                       (x, s))
        x = sum_div(rs, nk)
    x = leaky_relu(x, 0.01)  # F.leaky_relu's default slope (:569)
    cp = g.conv_post
    post = conv1d_frames(x, _wn_w(cp), cp.bias, 1, cp.padding, 1, dtype)  # [B, F, n_fft + 2]
    return cistft_head(post, st.weight_backward_real, st.weight_backward_imag, n_fft, hop)


def istft_decoder_forward(dec, asr, F0_curve, N, s, noise=None, seed=None, utt_offset=0, dtype="fp32"):
    """Decoder.forward (istftnet.py:692-721) with autograd through HIP kernels: asr [B, 512, T], F0_curve and
    N [B, 2T], s [B, style_dim] -> [B, 1, 2T prod(rates) hop].  `dec` is stts2_mi355x.istftnet.Decoder; in .train()
    mode the F0 / N smoothing of :693-701 is applied first (Python's random, as the reference).  `noise`
    [B, L, 9] / `seed` / `utt_offset` as for hifigan.Decoder.  The convs take `dtype` (fp32, bf16, bf16x3); the
    source, its STFT, the pad-add and the exp / sin -> inverse-STFT head are fp32 in all three."""
    _require_device()
    if dtype not in _DT:
        raise ValueError(f"dtype {dtype!r}: expected one of {list(_DT)}")
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if noise is None else 0
    if dec.training:
        F0_curve, N = train_smooth(F0_curve, N)
    # fp32 is the accuracy mode: its front-end convs are summed in 512-channel blocks (conv1d_chunked), since the
    # AdaIN1d's of a short front-end (T = 4: four frames per statistic) amplify the convs' rounding ~30x in d asr
    x = _decoder_frontend(dec, asr, F0_curve, N, s, dtype, kchunk=FRONT_KCHUNK if dtype == "fp32" else 0)
    return istft_generator_forward(dec.generator, x, s, F0_curve, noise, seed, utt_offset, dtype).unsqueeze(1)


# ---------------------------------------------------------------------- discriminators
def _k1_geom(layer):
    """(k, stride, pad) of a (k, 1) Conv2d: the reference's nn.Conv2d or training._WNConv2dK1."""
    if hasattr(layer, "kernel_size"):
        return layer.kernel_size[0], layer.stride[0], layer.padding[0]
    return layer.k, layer.stride, layer.pad


def discriminator_p_forward(m, x, period, dtype="fp32"):
    """DiscriminatorP.forward (discriminators.py:110-129) for a module with the reference's parameter layout:
    x [B, 1, T] -> (score [B, H*p], fmap: 6 maps [B, C, H, p], permuted views of frames [B*p, H, C])."""
    b, c, t = x.shape
    p = period
    if t % p != 0:
        x = torch.nn.functional.pad(x, (0, p - t % p), "reflect")  # discriminators.py:112-115
        t = x.shape[-1]
    h = x.reshape(b, c, t // p, p).permute(0, 3, 2, 1).reshape(b * p, t // p, c)
    fmap = []

    def nchw(f):
        return f.reshape(b, p, f.shape[1], f.shape[2]).permute(0, 3, 2, 1)

    for layer in m.convs:
        k, st, pad = _k1_geom(layer)
        w = _wn_w(layer)
        wk = w.reshape(w.shape[0], w.shape[1], k)
        if FUSE_LRELU:
            h = conv1d_frames(h, wk, layer.bias, st, pad, dtype=dtype, act_slope=0.1)
        else:
            h = leaky_relu(conv1d_frames(h, wk, layer.bias, st, pad, dtype=dtype), 0.1)
        fmap.append(nchw(h))
    cp = m.conv_post
    k, st, pad = _k1_geom(cp)
    w = _wn_w(cp)
    h = conv1d_frames(h, w.reshape(1, w.shape[1], k), cp.bias, st, pad, dtype=dtype)
    out = nchw(h)
    fmap.append(out)
    return torch.flatten(out, 1, -1), fmap


def spec_discriminator_forward(m, y, dtype="fp32"):
    """SpecDiscriminator.forward (discriminators.py:49-63) for the reference's parameter layout: y [B, 1, T]
    -> (score [B, F*W5], fmap: 6 maps [B, C, F, W], permuted views of frames [B, F, W, C]).  The |STFT|
    image is [B, F frames, nb bins]; each (3, kw) Conv2d is a 1-D conv along the bins over the 3 C
    time-expanded channels (x3[..., c*3 + dh] = row h + dh - 1), so the weight [Cout, C, 3, kw] is the
    [Cout, 3C, kw] conv1d weight as it lies in memory."""
    y = y.reshape(y.shape[0], -1)
    S = y.shape[0]
    h = stft_mag(y, m.fft_size, m.shift_size, m.win_length).unsqueeze(-1)  # [S, F, nb, 1]
    Fr = h.shape[1]
    fmap = []
    layers = list(m.discriminators) + [m.out]
    for j, layer in enumerate(layers):
        w = _wn_w(layer)
        co, ci, kh, kw = w.shape
        act = j < len(layers) - 1
        if (FUSE_TX and (FUSE_LRELU or not act) and ci == 32 and kh == 3 and layer.padding[0] == 1
                and layer.stride[0] == 1):
            out = _ConvTxFn.apply(h, w, layer.bias, layer.stride[1], layer.padding[1], dtype, 0.1 if act else None)
            h = out.reshape(S, Fr, out.shape[1], co)
            fmap.append(h.permute(0, 3, 1, 2))
            continue
        x3 = _TimeExpandFn.apply(h)  # [S, F, W, 3C]
        W3 = x3.shape[2]
        out = conv1d_frames(x3.reshape(S * Fr, W3, 3 * ci), w.reshape(co, ci * kh, kw), layer.bias,
                            layer.stride[1], layer.padding[1], dtype=dtype,
                            act_slope=0.1 if (act and FUSE_LRELU) else None)
        if act and not FUSE_LRELU:
            out = leaky_relu(out, 0.1)
        h = out.reshape(S, Fr, out.shape[1], co)
        fmap.append(h.permute(0, 3, 1, 2))
    return h.reshape(S, -1), fmap


# ------------------------------------------------------------------ dropout (train mode)
class _DropoutFn(torch.autograd.Function):
    """nn.Dropout(p) in train mode on the device (stts_dropout): the mask is a counter draw keyed by a seed from
    torch's default generator, redrawn (not stored) by the backward."""

    @staticmethod
    def forward(ctx, x, p):
        _require_device()
        xc = _c(x)
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        y = torch.empty_like(xc)
        call("stts_dropout", xc, xc.numel(), p, seed, y)
        ctx.p, ctx.seed = p, seed
        return y

    @staticmethod
    def backward(ctx, dy):
        dyc = _c(dy)
        dx = torch.empty_like(dyc)
        call("stts_dropout", dyc, dyc.numel(), ctx.p, ctx.seed, dx)
        return dx, None


class _DropoutMaskFn(torch.autograd.Function):
    """Train-mode dropout with an injected keep mask (stts_dropout_mask), forward and backward."""

    @staticmethod
    def forward(ctx, x, mask, p):
        _require_device()
        xc, mc = _c(x), _c(mask.to(x.device, torch.float32))
        if mc.shape != xc.shape:
            raise ValueError(f"dropout mask {tuple(mc.shape)} for a tensor {tuple(xc.shape)}")
        y = torch.empty_like(xc)
        call("stts_dropout_mask", xc, mc, xc.numel(), p, y)
        ctx.save_for_backward(mc)
        ctx.p = p
        return y

    @staticmethod
    def backward(ctx, dy):
        (mc,) = ctx.saved_tensors
        dyc = _c(dy)
        dx = torch.empty_like(dyc)
        call("stts_dropout_mask", dyc, mc, dyc.numel(), ctx.p, dx)
        return dx, None, None


_MASKS = {"fn": None, "k": 0}


def set_dropout_masks(fn):
    """Test hook: fn(k, shape, p) -> the keep mask (0 / 1, any device) of the k-th train-mode dropout call from now on,
    in the REFERENCE module's layout of that tensor (a call site whose layout differs passes ref_transpose); None
    goes back to the device counter draws.  The train-mode fixtures (tests/golden/make_golden_train_text.py) inject
    the same masks into the reference's F.dropout, so both sides drop the same elements."""
    _MASKS["fn"], _MASKS["k"] = fn, 0


def _next_mask(x, p, ref_transpose):
    """The injected keep mask of the next train-mode dropout call, laid out as x (None: the device counter draws)."""
    fn = _MASKS["fn"]
    if fn is None:
        return None
    shape = tuple(x.transpose(1, 2).shape) if ref_transpose else tuple(x.shape)
    m = torch.as_tensor(fn(_MASKS["k"], shape, float(p)), dtype=torch.float32, device=x.device)
    _MASKS["k"] += 1
    if ref_transpose:
        m = m.transpose(1, 2)
    return m.contiguous()


def dropout(x, p, ref_transpose=False):
    """nn.Dropout(p) / F.dropout in train mode.  ref_transpose: the reference holds this tensor as x.transpose(1, 2)
    (the TextEncoder's CNN, channels-first there), which is where an injected mask is laid out."""
    if p <= 0:
        return x
    m = _next_mask(x, p, ref_transpose)
    if m is None:
        return _DropoutFn.apply(x, float(p))
    return _DropoutMaskFn.apply(x, m, float(p))


# ------------------------------------------------------------------ the text aligner's conv stack (asr.ASRCNN)
def _drop_args(x, p, ref_transpose):
    """(p, seed, mask) of a fused train-mode dropout: the injected mask of this call, or a seed from torch's default
    generator for the counter draws (what _DropoutFn draws, so torch.manual_seed governs both)."""
    p = float(p)
    if p <= 0:
        return 0.0, 0, None
    m = _next_mask(x, p, ref_transpose)
    return p, (0 if m is not None else int(torch.randint(0, 2 ** 62, (1,)).item())), m


class _GroupNormFn(torch.autograd.Function):
    """dropout(GroupNorm(G)([ReLU] x)) on frames [B, L, C] with its backward: stts_groupnorm_fwd_train / _bwd.  The
    statistics are kept; the dropout is redrawn from the seed (or re-read from the injected mask) by the backward."""

    @staticmethod
    def forward(ctx, x, w, b, G, relu, p, seed, mask):
        _require_device()
        xc, wc, bc = _c(x), _c(w), _c(b)
        B, L, C = xc.shape
        if mask is not None and mask.shape != xc.shape:
            raise ValueError(f"dropout mask {tuple(mask.shape)} for a tensor {tuple(xc.shape)}")
        y = torch.empty_like(xc)
        stats = torch.empty(B, G, 2, dtype=torch.float32, device=xc.device)
        call("stts_groupnorm_fwd_train", xc, wc, bc, B, L, C, G, int(relu), p, seed, mask, y, stats,
             ws=("stts_groupnorm_fwd_train_workspace_bytes", B, L, C, G))
        ctx.save_for_backward(xc, wc, stats, mask)
        ctx.cfg = (G, int(relu), p, seed)
        return y

    @staticmethod
    def backward(ctx, gy):
        xc, wc, stats, mask = ctx.saved_tensors
        G, relu, p, seed = ctx.cfg
        B, L, C = xc.shape
        dy = _c(gy)
        nx, nw, nb = ctx.needs_input_grad[:3]
        dx = torch.empty_like(xc) if nx else None
        dw = torch.empty(C, dtype=torch.float32, device=dy.device) if nw else None
        db = torch.empty(C, dtype=torch.float32, device=dy.device) if nb else None
        call("stts_groupnorm_bwd", xc, wc, stats, dy, B, L, C, G, relu, p, seed, mask, dx, dw, db,
             ws=("stts_groupnorm_bwd_workspace_bytes", B, L, C, G))
        return dx, dw, db, None, None, None, None, None


def group_norm_frames(x, weight, bias, num_groups, relu=False, p=0.0, ref_transpose=False):
    """nn.GroupNorm(num_groups, C) of [ReLU of] frames x [B, L, C], then train-mode dropout(p) in the same launch
    (p = 0: none).  ref_transpose as for dropout()."""
    p, seed, m = _drop_args(x, p, ref_transpose)
    return _GroupNormFn.apply(x, weight, bias, int(num_groups), bool(relu), p, seed, m)


class _DropoutAddFn(torch.autograd.Function):
    """y = r + dropout(x) (stts_dropout_add_fwd); backward: dx = the same dropout of dy, dr = dy itself."""

    @staticmethod
    def forward(ctx, x, r, p, seed, mask):
        _require_device()
        xc, rc = _c(x), _c(r)
        if rc.shape != xc.shape or (mask is not None and mask.shape != xc.shape):
            raise ValueError(f"dropout + residual: x {tuple(xc.shape)}, r {tuple(rc.shape)}")
        y = torch.empty_like(xc)
        call("stts_dropout_add_fwd", xc, rc, xc.numel(), p, seed, mask, y)
        ctx.save_for_backward(mask)
        ctx.cfg = (p, seed)
        return y

    @staticmethod
    def backward(ctx, gy):
        (mask,) = ctx.saved_tensors
        p, seed = ctx.cfg
        nx, nr = ctx.needs_input_grad[:2]
        dx = None
        if nx:
            dy = _c(gy)
            if p <= 0:
                dx = dy
            else:
                dx = torch.empty_like(dy)
                if mask is not None:
                    call("stts_dropout_mask", dy, mask, dy.numel(), p, dx)
                else:
                    call("stts_dropout", dy, dy.numel(), p, seed, dx)
        return dx, (gy if nr else None), None, None, None


def dropout_add(x, r, p, ref_transpose=False):
    """r + dropout(x, p) in train mode, one launch (the ConvBlock tail `x = block(x); x += res`)."""
    p, seed, m = _drop_args(x, p, ref_transpose)
    return _DropoutAddFn.apply(x, r, p, seed, m)


def mfcc_frames(mel, dct_mat):
    """MFCC.forward on the device: mel [B, n_mels, T], dct_mat [n_mels, n_mfcc] -> frames [B, T, n_mfcc].  No
    gradient: the mel is data and dct_mat a buffer."""
    _require_device()
    mc, dc = _c(mel), _c(dct_mat)
    B, nm, T = mc.shape
    if dc.shape[0] != nm:
        raise ValueError(f"mfcc: mel {tuple(mc.shape)} against dct_mat {tuple(dc.shape)}")
    out = torch.empty(B, T, dc.shape[1], dtype=torch.float32, device=mc.device)
    call("stts_mfcc_frames", mc, dc, B, nm, T, dc.shape[1], out)
    return out


# ------------------------------------------------------------------ ProsodyPredictor.F0Ntrain (models.py:448-461)
class _BiLSTMFn(torch.autograd.Function):
    """Bidirectional nn.LSTM (batch_first) with its backward: stts_bilstm_fwd_train / stts_bilstm_bwd.  x frames
    [B, T, Cin]; ln: None (ProsodyPredictor.shared, full-length rows) or the device int32 text lengths (the packed
    sequences of the text / duration path, texttrain.py); params in torch's order."""

    @staticmethod
    def forward(ctx, x, ln, *params):
        _require_device()
        xc = _c(x)
        B, T, Cin = xc.shape
        ps = [_c(p) for p in params]
        H = ps[1].shape[1]
        arr = (ctypes.c_void_p * 8)(*[p.data_ptr() for p in ps])
        y = torch.empty(B, T, 2 * H, dtype=torch.float32, device=x.device)
        cs = torch.empty(2, B, T, H, dtype=torch.float32, device=x.device)
        call("stts_bilstm_fwd_train", xc, T * Cin, Cin, 1, B, T, Cin, ln, arr, H, y, cs,
             ws=("stts_bilstm_workspace_bytes", B, T, H))
        ctx.save_for_backward(xc, y, cs, ln if ln is not None else torch.empty(0), *ps)
        ctx.has_ln = ln is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        xc, y, cs, ln, *ps = ctx.saved_tensors
        ln = ln if ctx.has_ln else None
        B, T, Cin = xc.shape
        H = ps[1].shape[1]
        dyc = _c(dy)
        need = ctx.needs_input_grad
        dx = torch.empty_like(xc) if need[0] else None
        grads = [torch.empty_like(p) if need[i + 2] else None for i, p in enumerate(ps)]
        arr = (ctypes.c_void_p * 8)(*[p.data_ptr() for p in ps])
        garr = (ctypes.c_void_p * 8)(*[g.data_ptr() if g is not None else None for g in grads])
        call("stts_bilstm_bwd", xc, B, T, Cin, ln, arr, H, y, cs, dyc, dx, garr,
             ws=("stts_bilstm_bwd_workspace_bytes", B, T, Cin, H))
        return (dx, None, *grads)


def bilstm_frames(lstm, x):
    """lstm = the reference's nn.LSTM(.., bidirectional, batch_first) layout; x frames [B, T, Cin] -> [B, T, 2H]."""
    ps = [lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0, lstm.weight_ih_l0_reverse,
          lstm.weight_hh_l0_reverse, lstm.bias_ih_l0_reverse, lstm.bias_hh_l0_reverse]
    return _BiLSTMFn.apply(x, None, *ps)


def f0ntrain(pp, x, s, dtype="fp32"):
    """ProsodyPredictor.F0Ntrain (models.py:448-461) with autograd: x [B, d_hid + style_dim, T], s [B, style_dim]
    -> (F0 [B, 2T], N [B, 2T]).  The shared BiLSTM, the F0 / N AdainResBlk1d stacks (their dropout in train mode)
    and the 1x1 projections, on frames [B, T, C] throughout."""
    h = bilstm_frames(pp.shared, x.transpose(1, 2).contiguous())
    outs = []
    for blocks, proj in ((pp.F0, pp.F0_proj), (pp.N, pp.N_proj)):
        y = h
        for blk in blocks:
            y = adain_resblk1d_frames(blk, y, s, dtype)
        y = conv1d_frames(y, proj.weight, proj.bias, 1, 0, dtype=dtype)  # [B, 2T, 1]
        outs.append(y[..., 0])
    return outs[0], outs[1]


# ------------------------------------------------------------------ StyleEncoder (models.py:125-150)
class _RowExpFn(torch.autograd.Function):
    """Row expansion of a frames image [B, H, W, C] for a k x k Conv2d with H padding `pad`: [B, Ho, W, C k]."""

    @staticmethod
    def forward(ctx, x, k, pad):
        _require_device()
        xc = _c(x)
        B, H, W, C = xc.shape
        Ho = H + 2 * pad - k + 1
        xe = torch.empty(B, Ho, W, C * k, dtype=torch.float32, device=x.device)
        call("stts_rowexp_fwd", xc, B, H, W, C, k, pad, xe)
        ctx.geom = (B, H, W, C, k, pad)
        return xe

    @staticmethod
    def backward(ctx, dxe):
        B, H, W, C, k, pad = ctx.geom
        d = _c(dxe)
        dx = torch.empty(B, H, W, C, dtype=torch.float32, device=d.device)
        call("stts_rowexp_bwd", d, B, H, W, C, k, pad, dx)
        return dx, None, None


class _DWConvS2Fn(torch.autograd.Function):
    """LearnedDownSample('half'): depthwise Conv2d(C, C, 3, stride 2, pad 1) on frames images."""

    @staticmethod
    def forward(ctx, x, w, b):
        _require_device()
        xc, wc, bc = _c(x), _c(w), _c(b)
        B, H, W, C = xc.shape
        y = torch.empty(B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C, dtype=torch.float32, device=x.device)
        call("stts_dwconv2d_s2_fwd", xc, wc, bc, B, H, W, C, y)
        ctx.save_for_backward(xc, wc)
        ctx.has_b = b is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        xc, wc = ctx.saved_tensors
        B, H, W, C = xc.shape
        d = _c(dy)
        nx, nw, nb = ctx.needs_input_grad
        dx = torch.empty_like(xc) if nx else None
        dw = torch.empty_like(wc) if nw else None
        db = torch.empty(C, dtype=torch.float32, device=d.device) if (nb and ctx.has_b) else None
        call("stts_dwconv2d_s2_bwd", xc, wc, d, B, H, W, C, dx, dw, db, ws=("stts_dwconv2d_s2_workspace_bytes", C))
        return dx, dw, db


class _AvgPool2Fn(torch.autograd.Function):
    """DownSample('half') on frames images (the last column repeated when W is odd, then 2 x 2 averages)."""

    @staticmethod
    def forward(ctx, x):
        _require_device()
        xc = _c(x)
        B, H, W, C = xc.shape
        y = torch.empty(B, H // 2, (W + 1) // 2, C, dtype=torch.float32, device=x.device)
        call("stts_avgpool2_fwd", xc, B, H, W, C, y)
        ctx.geom = (B, H, W, C)
        return y

    @staticmethod
    def backward(ctx, dy):
        B, H, W, C = ctx.geom
        d = _c(dy)
        dx = torch.empty(B, H, W, C, dtype=torch.float32, device=d.device)
        call("stts_avgpool2_bwd", d, B, H, W, C, dx)
        return dx


class _SpatialMeanFn(torch.autograd.Function):
    """AdaptiveAvgPool2d(1) of a frames image [B, H, W, C] -> [B, C]."""

    @staticmethod
    def forward(ctx, x):
        _require_device()
        xc = _c(x)
        B, H, W, C = xc.shape
        y = torch.empty(B, C, dtype=torch.float32, device=x.device)
        call("stts_spatial_mean_fwd", xc, B, H * W, C, y)
        ctx.geom = (B, H, W, C)
        return y

    @staticmethod
    def backward(ctx, dy):
        B, H, W, C = ctx.geom
        d = _c(dy)
        dx = torch.empty(B, H, W, C, dtype=torch.float32, device=d.device)
        call("stts_spatial_mean_bwd", d, B, H * W, C, dx)
        return dx


def conv2d_frames(x, weight, bias, pad, dtype="fp32", residual=None, scale=1.0):
    """Conv2d(k x k, stride 1, padding pad) of a frames image x [B, H, W, Cin] with the reference weight
    [Cout, Cin, k, k]: the row expansion, then the conv1d engine over W (weight read as [Cout, Cin k, k]).
    residual (frames image of the output's shape) and scale ride in the conv's epilogue: (y + residual) * scale."""
    B, H, W, C = x.shape
    co, ci, k, kw = weight.shape
    if ci != C or kw != k:
        raise ValueError(f"conv2d_frames: weight {tuple(weight.shape)} for {C} input channels")
    xe = _RowExpFn.apply(x, k, pad) if k > 1 else x
    Ho = xe.shape[1]
    res = residual.reshape(B * Ho, residual.shape[2], co) if residual is not None else None
    y = conv1d_frames(xe.reshape(B * Ho, W, C * k), weight.reshape(co, C * k, k), bias, 1, pad, 1, dtype,
                      residual=res, scale=scale)
    return y.reshape(B, Ho, y.shape[1], co)


def style_encoder(se, mel, dtype="fp32"):
    """StyleEncoder.forward (models.py:145-150) with autograd: mel [B, 1, n_mels, F] -> [B, style_dim].
    shared = conv3x3 -> 4 x ResBlk('half': (DownSample(conv1x1(x)) + conv2(LReLU(LearnedDownSample(conv1(LReLU(x))))))
    / sqrt(2), models.py:82-123) -> LReLU -> conv5x5 (valid) -> AdaptiveAvgPool2d(1) -> LReLU; unshared = Linear.
    Frames images [B, n_mels, F, C] throughout."""
    blocks = list(se.shared)
    x = mel.permute(0, 2, 3, 1).contiguous()
    c0 = blocks[0]
    x = conv2d_frames(x, c0.weight, c0.bias, 1, dtype)
    for blk in blocks[1:5]:
        sc = x
        if blk.learned_sc:
            sc = conv2d_frames(sc, blk.conv1x1.weight, None, 0, dtype)
        sc = _AvgPool2Fn.apply(sc)
        r = conv2d_frames(leaky_relu(x, 0.2), blk.conv1.weight, blk.conv1.bias, 1, dtype)
        ds = blk.downsample_res.conv
        r = leaky_relu(_DWConvS2Fn.apply(r, ds.weight, ds.bias), 0.2)
        x = conv2d_frames(r, blk.conv2.weight, blk.conv2.bias, 1, dtype, residual=sc, scale=1 / math.sqrt(2))
    c5 = blocks[6]
    x = conv2d_frames(leaky_relu(x, 0.2), c5.weight, c5.bias, 0, dtype)
    h = leaky_relu(_SpatialMeanFn.apply(x), 0.2)
    return linear(h, se.unshared.weight, se.unshared.bias)
