"""Drop-in for Modules/ASR/models.py: ASRCNN, the text aligner of the training step.

train.py opens every iteration with `ppgs, s2s_pred, s2s_attn = model.text_aligner(mels, mask, texts)` (:206, and
:381 in validation).  This module holds the reference's 143 state-dict entries (so `load_state_dict(strict=True)`
takes a checkpoint's `text_aligner` block) and runs the eval-mode forward under no_grad on the HIP plan
(engine.AlignerEngine -> stts_aligner_fwd): the conv stack on the conv engines, the S2S attention decoder's
Tt + 1 steps as one persistent launch.

ASRS2S, the attention decoder, is trainable on its own: ASRS2S.forward runs stts_s2s_fwd_train / stts_s2s_bwd (back-
propagation through time in one persistent launch) under autograd, with losses.s2s_loss and losses.mono_loss.

The whole aligner trains when built with `ASRCNN(..., trainable=True)`: in train mode forward runs the same structure
as a composition under autograd (ASRCNN._features: the convs on training.conv1d_frames, GroupNorm with kept
statistics and the ConvBlock dropouts on stts_groupnorm_fwd_train / _bwd and stts_dropout_add_fwd, ctc_linear as K = 1
convs, the projection output handed to ASRS2S.forward as `memory`), and TrainStep(train_aligner=True) steps it.  The
keyword is opt-in: a default-built ASRCNN in train mode still raises (tests/test_aligner_cpu.py pins that), and in
eval mode both run the plan under no_grad, bit for bit alike.  Flipping the default is a later change.

`to_mfcc.dct_mat` is torchaudio's create_dct(40, 80, 'ortho'), computed here from its formula (torchaudio is not a
dependency); after load_state_dict the checkpoint's own buffer runs.
"""
from __future__ import annotations

import ctypes
import math

import torch
from torch import nn


def create_dct(n_mfcc: int, n_mels: int) -> torch.Tensor:
    """torchaudio.functional.create_dct(n_mfcc, n_mels, 'ortho'): [n_mels, n_mfcc] fp32."""
    n = torch.arange(float(n_mels))
    k = torch.arange(float(n_mfcc)).unsqueeze(1)
    dct = torch.cos(math.pi / float(n_mels) * (n + 0.5) * k)  # [n_mfcc, n_mels]
    dct[0] *= 1.0 / math.sqrt(2.0)
    dct *= math.sqrt(2.0 / float(n_mels))
    return dct.t().contiguous()


class MFCC(nn.Module):
    def __init__(self, n_mfcc=40, n_mels=80):
        super().__init__()
        self.n_mfcc, self.n_mels, self.norm = n_mfcc, n_mels, "ortho"
        self.register_buffer("dct_mat", create_dct(n_mfcc, n_mels))


class LinearNorm(nn.Module):
    def __init__(self, in_dim, out_dim, bias=True, w_init_gain="linear"):
        super().__init__()
        self.linear_layer = nn.Linear(in_dim, out_dim, bias=bias)
        nn.init.xavier_uniform_(self.linear_layer.weight, gain=nn.init.calculate_gain(w_init_gain))


class ConvNorm(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size=1, stride=1, padding=None, dilation=1, bias=True):
        super().__init__()
        if padding is None:
            padding = dilation * (kernel_size - 1) // 2
        self.conv = nn.Conv1d(in_channels, out_channels, kernel_size=kernel_size, stride=stride, padding=padding,
                              dilation=dilation, bias=bias)
        nn.init.xavier_uniform_(self.conv.weight, gain=nn.init.calculate_gain("linear"))


class ConvBlock(nn.Module):
    """reference Modules/ASR/layers.py:105-131 (parameter layout)."""

    def __init__(self, hidden_dim, n_conv=3, dropout_p=0.2):
        super().__init__()
        self.blocks = nn.ModuleList([nn.Sequential(
            ConvNorm(hidden_dim, hidden_dim, kernel_size=3, padding=3 ** i, dilation=3 ** i),
            nn.ReLU(),
            nn.GroupNorm(num_groups=8, num_channels=hidden_dim),
            nn.Dropout(p=dropout_p),
            ConvNorm(hidden_dim, hidden_dim, kernel_size=3, padding=1, dilation=1),
            nn.ReLU(),
            nn.Dropout(p=dropout_p)) for i in range(n_conv)])


class LocationLayer(nn.Module):
    def __init__(self, n_filters, kernel_size, attention_dim):
        super().__init__()
        self.location_conv = ConvNorm(2, n_filters, kernel_size=kernel_size, padding=(kernel_size - 1) // 2,
                                      bias=False)
        self.location_dense = LinearNorm(n_filters, attention_dim, bias=False, w_init_gain="tanh")


class Attention(nn.Module):
    def __init__(self, rnn_dim, embedding_dim, attention_dim, n_filters, kernel_size):
        super().__init__()
        self.query_layer = LinearNorm(rnn_dim, attention_dim, bias=False, w_init_gain="tanh")
        self.memory_layer = LinearNorm(embedding_dim, attention_dim, bias=False, w_init_gain="tanh")
        self.v = LinearNorm(attention_dim, 1, bias=False)
        self.location_layer = LocationLayer(n_filters, kernel_size, attention_dim)


class ASRS2S(nn.Module):
    """reference Modules/ASR/models.py:74-100 (parameter layout)."""

    def __init__(self, embedding_dim=256, hidden_dim=512, n_location_filters=32, location_kernel_size=63, n_token=40):
        super().__init__()
        self.embedding = nn.Embedding(n_token, embedding_dim)
        val_range = math.sqrt(6 / hidden_dim)
        self.embedding.weight.data.uniform_(-val_range, val_range)
        self.decoder_rnn_dim = hidden_dim
        self.project_to_n_symbols = nn.Linear(hidden_dim, n_token)
        self.attention_layer = Attention(hidden_dim, hidden_dim, hidden_dim, n_location_filters, location_kernel_size)
        self.decoder_rnn = nn.LSTMCell(hidden_dim + embedding_dim, hidden_dim)
        self.project_to_hidden = nn.Sequential(LinearNorm(hidden_dim * 2, hidden_dim), nn.Tanh())
        self.sos, self.eos, self.unk_index, self.random_mask = 1, 2, 3, 0.1
        self.n_token, self.embedding_dim = n_token, embedding_dim

    def forward(self, memory, memory_mask, text_input, unk_mask=None):
        """reference models.py:118-147: memory [B, L, 128], memory_mask bool [B, L] (True = padded) or None,
        text_input [B, Tt] -> (hidden [B, Tt + 1, 128], logit [B, Tt + 1, n_token], alignments [B, Tt + 1, L]).
        With grad mode on and a parameter or `memory` requiring grad, the autograd path (all three outputs take
        upstream gradients); in train mode F.dropout(hidden, 0.5) of :174 is training.dropout (device counter draws,
        or the masks of training.set_dropout_masks).  unk_mask (bool [B, Tt]): the tokens replaced by the unknown
        index, drawn on the host as the reference does when None."""
        from .texttrain import needs_grad
        if self.decoder_rnn_dim != 128 or self.attention_layer.location_layer.location_conv.conv.weight.shape != (
                32, 2, 63):
            raise NotImplementedError("ASRS2S: the HIP decoder is built for hidden_dim = 128, 32 location filters of "
                                      "63 taps (the reference's)")
        tok = text_input.detach().cpu()
        if tok.dim() != 2 or tok.shape[1] < 1:
            raise ValueError(f"ASRS2S: text_input must be [B, Tt >= 1], got {tuple(tok.shape)}")
        if int(tok.min()) < 0 or int(tok.max()) >= self.n_token:
            raise IndexError(f"ASRS2S: token indices must lie in [0, {self.n_token})")
        if unk_mask is None:
            unk_mask = torch.rand(text_input.shape) < self.random_mask
        dev = memory.device
        B, L, _ = memory.shape
        steps = tok.shape[1] + 1
        scale = None
        if self.training:
            from .training import dropout
            scale = dropout(torch.ones(B, steps, 128, dtype=torch.float32, device=dev), 0.5).detach()
        um = unk_mask.to(device=dev, dtype=torch.uint8).contiguous()
        mm = None if memory_mask is None else memory_mask.to(device=dev, dtype=torch.uint8).contiguous()
        tk = tok.to(device=dev, dtype=torch.int32).contiguous()
        params = [p for _, p in self.named_parameters()]
        if needs_grad(self, memory):
            return _S2SFn.apply(memory, mm, tk, um, scale, *params)
        with torch.no_grad():
            return _s2s_forward(memory, mm, tk, um, scale, params, save=False)[:3]


def _s2s_forward(memory, mm, tk, um, scale, params, save):
    from .engine import _require_device, call, query
    _require_device()
    mc = memory.detach().to(torch.float32).contiguous()
    ps = [p.detach().to(torch.float32).contiguous() for p in params]
    B, L, D = mc.shape
    Tt = tk.shape[1]
    ntok, E = ps[0].shape
    if D != 128 or len(ps) != 14:
        raise ValueError(f"ASRS2S: memory must be [B, L, 128], got {tuple(mc.shape)}")
    dev = mc.device
    hidden = torch.empty(B, Tt + 1, D, dtype=torch.float32, device=dev)
    logit = torch.empty(B, Tt + 1, ntok, dtype=torch.float32, device=dev)
    attn = torch.empty(B, Tt + 1, L, dtype=torch.float32, device=dev)
    sv = torch.empty(query("stts_s2s_save_bytes", B, L, Tt), dtype=torch.uint8, device=dev) if save else None
    arr = (ctypes.c_void_p * 14)(*[p.data_ptr() for p in ps])
    call("stts_s2s_fwd_train", mc, mm, tk, um, arr, B, L, Tt, ntok, E, scale, hidden, logit, attn, sv,
         ws=("stts_s2s_fwd_train_workspace_bytes", B, L, Tt, ntok, E))
    return hidden, logit, attn, sv, mc, ps


class _S2SFn(torch.autograd.Function):
    """ASRS2S.forward with its backward: stts_s2s_fwd_train / stts_s2s_bwd.  Inputs after the five data tensors: the
    14 parameters in named_parameters() order."""

    @staticmethod
    def forward(ctx, memory, mm, tk, um, scale, *params):
        hidden, logit, attn, sv, mc, ps = _s2s_forward(memory, mm, tk, um, scale, params, save=True)
        none = torch.empty(0)
        ctx.save_for_backward(mc, mm if mm is not None else none, tk, um, scale if scale is not None else none,
                              hidden, attn, sv, *ps)
        ctx.has = (mm is not None, scale is not None)
        return hidden, logit, attn

    @staticmethod
    def backward(ctx, dhidden, dlogit, dattn):
        from .engine import call
        mc, mm, tk, um, scale, hidden, attn, sv, *ps = ctx.saved_tensors
        mm = mm if ctx.has[0] else None
        scale = scale if ctx.has[1] else None
        B, L, D = mc.shape
        Tt = tk.shape[1]
        ntok, E = ps[0].shape
        need = ctx.needs_input_grad
        f32 = lambda t: None if t is None else t.to(torch.float32).contiguous()  # noqa: E731
        dmem = torch.empty_like(mc) if need[0] else None
        grads = [torch.empty_like(p) if need[5 + i] else None for i, p in enumerate(ps)]
        arr = (ctypes.c_void_p * 14)(*[p.data_ptr() for p in ps])
        garr = (ctypes.c_void_p * 14)(*[g.data_ptr() if g is not None else None for g in grads])
        call("stts_s2s_bwd", mc, mm, tk, um, arr, B, L, Tt, ntok, E, scale, hidden, attn, sv, f32(dhidden),
             f32(dlogit), f32(dattn), dmem, garr, ws=("stts_s2s_bwd_workspace_bytes", B, L, Tt, ntok, E))
        return (dmem, None, None, None, None, *grads)


class ASRCNN(nn.Module):
    """reference Modules/ASR/models.py:8-72.  `trainable=True` (a constructor keyword, not part of the state dict)
    allows train mode: forward and get_feature then run the autograd composition (_features) instead of the plan."""

    def __init__(self, input_dim=80, hidden_dim=256, n_token=35, n_layers=6, token_embedding_dim=256,
                 trainable=False):
        super().__init__()
        self.n_token = n_token
        self.n_down = 1
        self.trainable = bool(trainable)
        self.cfg = [input_dim, hidden_dim, n_token, n_layers, token_embedding_dim]
        self.to_mfcc = MFCC()
        self.init_cnn = ConvNorm(input_dim // 2, hidden_dim, kernel_size=7, padding=3, stride=2)
        self.cnns = nn.Sequential(*[nn.Sequential(ConvBlock(hidden_dim), nn.GroupNorm(num_groups=1,
                                                                                      num_channels=hidden_dim))
                                    for _ in range(n_layers)])
        self.projection = ConvNorm(hidden_dim, hidden_dim // 2)
        self.ctc_linear = nn.Sequential(LinearNorm(hidden_dim // 2, hidden_dim), nn.ReLU(),
                                        LinearNorm(hidden_dim, n_token))
        self.asr_s2s = ASRS2S(embedding_dim=token_embedding_dim, hidden_dim=hidden_dim // 2, n_token=n_token)
        self._engine = None

    def invalidate(self):
        """Drop the packed weights (after writes through `param.data`, which stale() cannot see)."""
        self._engine = None

    def engine(self, dtype="fp32"):
        from .engine import AlignerEngine
        if self._engine is None or self._engine.dtype != dtype or self._engine.stale(self):
            self._engine = AlignerEngine(self, dtype=dtype)
        return self._engine

    def _check(self):
        if self.training and not self.trainable:
            raise NotImplementedError("ASRCNN: built with trainable=False, the HIP path is the eval-mode forward under "
                                      "no_grad; build it with ASRCNN(..., trainable=True) to run train mode (the "
                                      "autograd composition), or call .eval() first")
        if self.cfg[0] != 80 or self.cfg[1] != 256:
            raise NotImplementedError("ASRCNN: the HIP plan is built for input_dim = 80, hidden_dim = 256 (the "
                                      "reference's)")

    def _features(self, x, dtype="fp32"):
        """Train mode (trainable=True): mel [B, 80, T] -> the projection output as frames [B, L, 128], the eval
        plan's structure (plan.cpp:aligner_forward) as a composition under autograd: MFCC, init_cnn, 6 x [3 x
        (conv + ReLU -> GroupNorm(8) + dropout -> conv + ReLU -> dropout + input) -> GroupNorm(1)], projection.  A
        ConvBlock entry is four launches forward (training.conv1d_frames with act_slope 0, group_norm_frames,
        dropout_add).  The 36 dropouts are drawn on the device, or taken from training.set_dropout_masks in the
        reference's call order and [B, 256, L] layout.  The mel gets no gradient: it is data (stts_mfcc_frames has no
        backward)."""
        from . import training as Tr
        if dtype != "fp32":
            raise NotImplementedError("ASRCNN: train mode runs in fp32")
        if not x.is_cuda:
            raise RuntimeError("ASRCNN: train mode needs the input on a HIP device; no CPU fallback exists")
        h = Tr.mfcc_frames(x, self.to_mfcc.dct_mat)
        c = self.init_cnn.conv
        h = Tr.conv1d_frames(h, c.weight, c.bias, stride=2, padding=3)
        for layer in self.cnns:
            for blk in layer[0].blocks:
                c1, gn, c2 = blk[0].conv, blk[2], blk[4].conv
                t = Tr.conv1d_frames(h, c1.weight, c1.bias, padding=c1.padding[0], dilation=c1.dilation[0],
                                     act_slope=0.0)
                t = Tr.group_norm_frames(t, gn.weight, gn.bias, gn.num_groups, p=blk[3].p, ref_transpose=True)
                t = Tr.conv1d_frames(t, c2.weight, c2.bias, padding=c2.padding[0], act_slope=0.0)
                h = Tr.dropout_add(t, h, blk[6].p, ref_transpose=True)
            gn = layer[1]
            h = Tr.group_norm_frames(h, gn.weight, gn.bias, gn.num_groups)
        c = self.projection.conv
        return Tr.conv1d_frames(h, c.weight, c.bias)

    def _ctc(self, feat):
        """ctc_linear (Linear, ReLU, Linear) over frames [B, L, 128] as K = 1 convs."""
        from . import training as Tr
        l1, l2 = self.ctc_linear[0].linear_layer, self.ctc_linear[2].linear_layer
        h = Tr.conv1d_frames(feat, l1.weight.unsqueeze(-1), l1.bias, act_slope=0.0)
        return Tr.conv1d_frames(h, l2.weight.unsqueeze(-1), l2.bias)

    def draw_unk_mask(self, text_input):
        """models.py:126: the 10 % unknown-token draw, on the host as the reference's, so torch.manual_seed
        reproduces it."""
        return torch.rand(text_input.shape) < self.asr_s2s.random_mask

    def forward(self, x, src_key_padding_mask=None, text_input=None, dtype="fp32", unk_mask=None):
        """mel [B, 80, T] -> ctc_logit [B, L, n_token], or with text_input [B, Tt] (ctc_logit, s2s_logit
        [B, Tt + 1, n_token], s2s_attn [B, Tt + 1, L]); L = ceil(T / 2).  unk_mask (bool [B, Tt]): the tokens
        replaced by the unknown index, drawn as the reference does when None.  In train mode (trainable=True) the
        outputs carry the autograd graph of _features, ctc_linear and ASRS2S.forward (the projection output is the
        decoder's `memory`, so its dmemory flows back into the conv stack); eval mode runs the plan under no_grad."""
        self._check()
        if self.training:
            feat = self._features(x, dtype)
            ctc = self._ctc(feat)
            if text_input is None:
                return ctc
            if unk_mask is None:
                unk_mask = self.draw_unk_mask(text_input)
            _, s2s, attn = self.asr_s2s(feat, src_key_padding_mask, text_input, unk_mask=unk_mask)
            return ctc, s2s, attn
        if text_input is None:
            with torch.no_grad():
                return self.engine(dtype).forward(x, s2s=False, attn=False)[0]
        tok = text_input.detach().cpu()
        if tok.numel() and (int(tok.min()) < 0 or int(tok.max()) >= self.n_token):
            raise IndexError(f"ASRCNN: token indices must lie in [0, {self.n_token})")
        if unk_mask is None:
            unk_mask = self.draw_unk_mask(text_input)
        with torch.no_grad():
            ctc, s2s, attn, _ = self.engine(dtype).forward(x, src_key_padding_mask, text_input, unk_mask)
        return ctc, s2s, attn

    def get_feature(self, x, dtype="fp32"):
        """The projection output [B, 128, L] (models.py:50-55)."""
        self._check()
        if self.training:
            return self._features(x.squeeze(1) if x.dim() == 4 else x, dtype).transpose(1, 2)
        with torch.no_grad():
            return self.engine(dtype).forward(x.squeeze(1) if x.dim() == 4 else x, ctc=False, feature=True)[3]

    def length_to_mask(self, lengths):
        mask = torch.arange(lengths.max()).unsqueeze(0).expand(lengths.shape[0], -1).type_as(lengths)
        return torch.gt(mask + 1, lengths.unsqueeze(1)).to(lengths.device)
