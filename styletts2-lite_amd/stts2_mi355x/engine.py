"""ctypes binding of libstts2.so (include/stts2.h) and the per-module engines.

PyTorch is used only as the device-memory / stream container: parameters are the
module's own state-dict tensors on the HIP device, the packed-weight buffer and the
workspace are torch uint8 tensors, and every kernel is launched by the C library on
`torch.cuda.current_stream()`.  There is no compute fallback: without the library or
a HIP device every call raises.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np
import torch

from .abi import SIGNATURES

KIND_HIFIGAN, KIND_ISTFTNET, KIND_F0N, KIND_STYLE, KIND_MPD, KIND_VOCOS, KIND_MSD = 0, 1, 2, 3, 4, 5, 6
KIND_PITCH = 8  # (7 is not a kind: include/stts2.h)
KIND_ALIGNER = 9
DTYPES = {"fp32": 0, "bf16": 1, "bf16x3": 2}  # bf16x3: the split-operand accuracy mode (STTS_SPLIT)

_LIB = None
_HERE = os.path.dirname(os.path.abspath(__file__))
# (STTS_LIB: another build of the same C-ABI revision, for build-against-build A/Bs on one box: tools/gpu/)
LIB_PATH = os.environ.get("STTS_LIB") or os.path.join(_HERE, "libstts2.so")
ABI_VERSION = 5  # include/stts2.h STTS_ABI_VERSION: the revision abi.SIGNATURES describes

c_int, c_ll, c_vp = ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p


def lib():
    """Load libstts2.so (after torch, so both share torch's HIP runtime) and give every entry point its signature
    (abi.SIGNATURES): the one place the library is bound, whichever module calls it."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} missing: build it with `python -m stts2_mi355x.build` "
                           "(__graft_entry__.build()); there is no non-HIP fallback")
    L = ctypes.CDLL(LIB_PATH)
    # (an int return and no arguments are ctypes' defaults, so the revision is read before the table is applied)
    rev = L.stts_abi_version() if hasattr(L, "stts_abi_version") else None
    if rev != ABI_VERSION:
        raise RuntimeError(f"{LIB_PATH}: C-ABI revision {rev}, these bindings expect {ABI_VERSION} "
                           "(include/stts2.h STTS_ABI_VERSION): rebuild the library")
    for name, (args, res) in SIGNATURES.items():
        fn = getattr(L, name, None)
        if fn is None:
            raise RuntimeError(f"{LIB_PATH} does not export {name} (include/*.h declares it): rebuild the library")
        fn.argtypes, fn.restype = args, res
    _LIB = L
    if os.environ.get("STTS_OPTS"):
        for k, v in OPT_DEFAULTS.items():
            call("stts_set_option", int(k), int(v))
    return L


# (name, key, production default) of every live STTS_OPT_* (include/stts2.h; csrc/options.h holds the library's rows).
# Keys 3, 9, 26 and 28 are retired and never reused.
_OPTS = (("RESCONV", 1, 1), ("GRID_CAP", 2, 0), ("DEBUG", 4, 0), ("STATS_SLOTS", 5, 0), ("SMALL_TILES", 6, 1),
         ("BIGCONV", 7, 2), ("HEAD", 8, 1), ("FRONT", 10, 1), ("PW", 11, 1), ("SPLITK", 12, 1), ("EXP", 13, 0),
         ("UPS", 14, 1), ("WGRAD", 15, 1), ("PLAINRC", 16, 1), ("MSDFOLD", 17, 1), ("RCPP", 18, 3), ("RESSPLIT", 19, 1),
         ("BF16F", 20, 0), ("YF32", 21, 1), ("COUT1", 22, 1), ("BRANCHES", 23, 8), ("NBRANCH", 24, 64),
         ("BIGSPLIT", 25, 1), ("BIG64", 27, 5), ("SEGPART", 29, 1), ("RCOCC", 30, 1))
globals().update({"OPT_" + _n: _k for _n, _k, _ in _OPTS})  # OPT_RESCONV = 1, ...
OPT_DEFAULTS = {_k: _d for _, _k, _d in _OPTS}
# STTS_OPTS="KEY=VALUE,..." (A/B runs of whole suites): option values that replace the defaults for the process,
# applied when the library loads and by reset_options()
for _kv in filter(None, os.environ.get("STTS_OPTS", "").split(",")):
    _k, _v = (int(x) for x in _kv.split("="))
    OPT_DEFAULTS[_k] = _v


def set_option(key: int, value: int) -> None:
    """Process-wide engine option (include/stts2.h STTS_OPT_*)."""
    call("stts_set_option", int(key), int(value))


def get_option(key: int) -> int:
    return int(lib().stts_get_option(int(key)))


def reset_options() -> None:
    """Every engine option back to its production default (tests restore this after A/B runs)."""
    if _LIB is None:
        return
    for k, v in OPT_DEFAULTS.items():
        set_option(k, v)
    from . import prosody
    prosody.set_lstm_group(0)
    prosody.set_bilstm_debug(0, False)


def check(rc: int, what: str = "stts"):
    if rc != 0:
        msg = lib().stts_error_string(rc).decode()
        raise RuntimeError(f"{what} failed: {msg} (code {rc})")


def forward_only(module, what):
    """The HIP path of `module` has no backward: refuse to run where the caller would differentiate the
    output (grad mode on and a parameter requiring grad), instead of returning a tensor without a graph
    whose gradients would silently be lost.  Inference runs under torch.no_grad() (inference.py:234)."""
    if torch.is_grad_enabled() and any(p.requires_grad for p in module.parameters()):
        raise NotImplementedError(
            f"{what}: the HIP path is forward-only (no backward kernels for this module); call it under "
            "torch.no_grad() as inference.py does, or freeze its parameters (requires_grad_(False))")


_DEVICE_OK = False


def _require_device():
    global _DEVICE_OK
    if _DEVICE_OK:
        return
    if not torch.cuda.is_available():
        raise RuntimeError("stts2_mi355x needs a HIP device (MI355X / gfx950); no CPU fallback exists")
    _DEVICE_OK = True


# the raw query of the current stream: torch.cuda.current_stream() costs ~9 us of host time a call (device index,
# availability and environment checks), and a training step makes ~2,500 of these calls
_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_GET_DEVICE = getattr(torch._C, "_cuda_getDevice", None)


def _stream():
    """The current HIP stream's handle as an int (the entry points' argtypes make it the hipStream_t)."""
    if _RAW_STREAM is not None and _GET_DEVICE is not None:
        return _RAW_STREAM(_GET_DEVICE())
    return torch.cuda.current_stream().cuda_stream  # (a torch without the raw query)


def _ptr(t):
    """A tensor (or None) as a c_void_p: for the tests and tools that call lib() directly; the package uses call()."""
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def query(name, *args):
    """A size query (*_workspace_bytes, *_out_elems, *_scratch_bytes, ...: they return long long and take no stream):
    its value; a negative one is the query's STTS_E* code for these arguments and raises.  Needs no device."""
    n = int(getattr(lib(), name)(*args))
    if n < 0:
        check(n, name)
    return n


def _workspace(query_name: str, device, *args):
    """(buffer, bytes) for a kernel whose size query is query(query_name, *args): for call sites that share one
    buffer between calls or pass it elsewhere than right before the stream; the others say call(..., ws=(...))."""
    nbytes = query(query_name, *args)
    return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device), nbytes


_ENTRIES = {}  # name -> _bind(name), built on the entry point's first call


def _bind(name, fn=None):
    """run(args, ws) for one status-returning entry point, built once from its abi.SIGNATURES row (`fn` replaces the
    library's function: tests).  A tensor at a c_void_p position goes as its data_ptr(); None stays None, ctypes' NULL;
    anything else (model handles, ctypes arrays, byref(), ints, floats) is left to argtypes.  One argument fewer than
    the signature: the current stream is appended.  ws = (query name, *query args): the workspace is sized by that
    query, allocated on the device of the first tensor argument and passed as (buffer, bytes) right before the
    stream.  Any other argument count raises before anything is launched; a non-zero status raises as check()."""
    argtypes, restype = SIGNATURES[name]
    if restype is not c_int:
        raise TypeError(f"{name} returns no status: query() serves the size queries")
    n = len(argtypes)
    ptrs = tuple(i for i, t in enumerate(argtypes) if t is c_vp)
    ends_in_ptr = n > 0 and argtypes[-1] is c_vp  # where a stream can be
    takes_ws = list(argtypes[-3:]) == [c_vp, c_ll, c_vp]
    cache = fn is None
    if cache:
        fn = getattr(lib(), name)
    Tensor = torch.Tensor

    def run(args, ws=None):
        given = len(args)
        if ws is not None:
            if not takes_ws:
                raise TypeError(f"{name} does not end in (workspace, bytes, stream): pass the workspace explicitly")
            if given != n - 3:
                raise TypeError(f"{name} takes {n} arguments, got {given} + workspace, bytes and stream (ws=)")
            dev = next((args[i].device for i in ptrs[:-2] if isinstance(args[i], Tensor)), None)
            if dev is None:
                raise TypeError(f"{name}: ws= puts the workspace on the first tensor argument's device; there is none")
            a = [*args, *_workspace(ws[0], dev, *ws[1:]), _stream()]
        elif given == n:
            a = list(args)
        elif given == n - 1 and ends_in_ptr:
            a = [*args, _stream()]
        else:
            raise TypeError(f"{name} takes {n} arguments" + (" (the stream may be left out)" if ends_in_ptr else "")
                            + f", got {given}")
        for i in ptrs:
            v = a[i]
            if isinstance(v, Tensor):
                a[i] = v.data_ptr()
        rc = fn(*a)
        if rc != 0:
            check(rc, name)

    if cache:
        _ENTRIES[name] = run
    return run


def call(name, *args, ws=None):
    """Call the entry point `name` of the library (see _bind): call("stts_snake_bwd", xc, ac, dyc, B, L, C, dx, da,
    ws=("stts_snake_workspace_bytes", B, L, C)).  A new entry point needs its abi.SIGNATURES row and nothing else."""
    (_ENTRIES.get(name) or _bind(name))(args, ws)


def _dev_f32(t, device):
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(np.asarray(t))
    return t.detach().to(device=device, dtype=torch.float32).contiguous()


class NativeModel:
    """One stts_model handle: parameters bound by reference state-dict name, packed per dtype."""

    def __init__(self, kind: int, cfg, module: torch.nn.Module):
        _require_device()
        L = lib()
        self.kind = kind
        arr = (c_int * len(cfg))(*[int(v) for v in cfg])
        h = c_vp()
        call("stts_model_create", kind, arr, len(cfg), ctypes.byref(h))
        self.h = h
        self.device = torch.device("cuda", torch.cuda.current_device())
        sd = module.state_dict(keep_vars=True)
        n = L.stts_param_count(h)
        self.names, self._keep = [], []
        # (tensor, _version, data_ptr) of every bound module tensor: an in-place update, a .to() or a
        # load_state_dict makes the packed weights stale (_Engine.stale)
        self.sources = []
        for i in range(n):
            name = L.stts_param_name(h, i).decode()
            if name not in sd:
                raise KeyError(f"parameter {name} expected by the native plan is not in the module state dict")
            src = sd[name]
            self.sources.append((src, src._version, src.data_ptr()))
            t = _dev_f32(src.detach(), self.device)
            if t.numel() != L.stts_param_numel(h, i):
                raise ValueError(f"{name}: numel {t.numel()} != plan {L.stts_param_numel(h, i)}")
            self._keep.append(t)
            self.names.append(name)
            call("stts_set_param", h, i, t)
        self._packed = {}
        self._ws = {}

    def pack(self, dtype: str):
        if dtype not in self._packed:
            dt = DTYPES[dtype]
            nb = query("stts_packed_bytes", self.h, dt)
            buf = torch.empty(max(nb, 1), dtype=torch.uint8, device=self.device)
            call("stts_pack", self.h, dt, buf, nb)
            self._packed[dtype] = buf
        return self._packed[dtype]

    def workspace(self, dtype: str, B: int, T: int):
        nb = query("stts_workspace_bytes", self.h, DTYPES[dtype], int(B), int(T))
        cur = self._ws.get(dtype)
        if cur is None or cur.numel() < nb:
            self._ws[dtype] = cur = torch.empty(max(nb, 1), dtype=torch.uint8, device=self.device)
        return cur, nb

    def __del__(self):
        try:
            if getattr(self, "h", None) and _LIB is not None:
                _LIB.stts_model_destroy(self.h)
        except Exception:
            pass


def _watch(module, engine_attr="_engine"):
    """Drop a module's cached engine whenever new weights are loaded."""
    if getattr(module, "_stts_hooked", False):
        return

    def hook(mod, incompatible):
        setattr(mod, engine_attr, None)
    module.register_load_state_dict_post_hook(hook)
    module._stts_hooked = True


class _Engine:
    def __init__(self, module, dtype):
        if dtype not in DTYPES:
            raise ValueError(f"dtype must be one of {list(DTYPES)}")
        self.dtype = dtype
        _watch(module)

    def stale(self, module):
        """True when a bound parameter changed since packing: an in-place update (its _version moved),
        a move or re-allocation (.to(), .cuda(), a new tensor: data_ptr moved).  Writes through
        `param.data` bypass the version counter: call `module.invalidate()` after those."""
        for src, ver, ptr in self.model.sources:
            if src._version != ver or src.data_ptr() != ptr:
                return True
        return False


class DecoderEngine(_Engine):
    """HIP forward of Modules/hifigan.py / istftnet.py / vocos.py Decoder (reference :446 / :692 / :392)."""

    def __init__(self, module, dtype="fp32"):
        super().__init__(module, dtype)
        g = module.generator
        if module.decoder_type == "vocos":
            kind = KIND_VOCOS
            cfg = [module.dim_in, module.style_dim, g.intermediate_dim, g.num_layers, g.n_fft, g.hop]
            self.scale = g.hop  # output samples per F0 frame (2T frames x hop)
        else:
            kind = KIND_ISTFTNET if module.decoder_type == "istftnet" else KIND_HIFIGAN
            cfg = [module.dim_in, module.style_dim, g.upsample_initial_channel, len(g.upsample_rates),
                   *g.upsample_rates, *g.upsample_kernel_sizes, len(g.resblock_kernel_sizes),
                   *g.resblock_kernel_sizes, *[d for ds in g.resblock_dilation_sizes for d in ds]]
            if kind == KIND_ISTFTNET:
                cfg += [g.gen_istft_n_fft, g.gen_istft_hop_size]
            self.scale = g.upsample_scale
        self.kind = kind
        self.dim_in, self.style_dim = module.dim_in, module.style_dim
        self.model = NativeModel(kind, cfg, module)
        self.model.pack(dtype)

    def forward(self, asr, F0_curve, N, s, noise=None, seed=None, utt_offset=0, out=None):
        """seed None (and no noise): one draw from torch's default generator keys the device noise,
        so torch.manual_seed governs it and successive calls differ, as the reference's
        randn_like draws (hifigan.py:213) do."""
        dev = self.model.device
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if noise is None and self.kind != KIND_VOCOS else 0
        in_dev = asr.device if isinstance(asr, torch.Tensor) else torch.device("cpu")
        asr, F0_curve, N, s = (_dev_f32(t, dev) for t in (asr, F0_curve, N, s))
        B, C, T = asr.shape
        if C != self.dim_in or tuple(F0_curve.shape) != (B, 2 * T) or tuple(N.shape) != (B, 2 * T) \
                or tuple(s.shape) != (B, self.style_dim):
            raise ValueError(f"decoder inputs: asr {tuple(asr.shape)}, F0 {tuple(F0_curve.shape)}, "
                             f"N {tuple(N.shape)}, s {tuple(s.shape)}")
        if T < 2:  # the reference's InstanceNorm1d raises on a single frame (torch F.instance_norm)
            raise ValueError(f"decoder inputs: need at least 2 asr frames, got {T}")
        Lw = 2 * T * self.scale
        if noise is not None and self.kind == KIND_VOCOS:
            raise ValueError("the Vocos decoder has no harmonic source: noise must be None")
        if noise is not None:
            noise = _dev_f32(noise, dev)
            if tuple(noise.shape) != (B, Lw, 9):
                raise ValueError(f"noise must be [B, {Lw}, 9], got {tuple(noise.shape)}")
        if out is None:
            out = torch.empty(B, 1, Lw, dtype=torch.float32, device=dev)
        ws, nb = self.model.workspace(self.dtype, B, T)
        call("stts_decoder_fwd", self.model.h, DTYPES[self.dtype], asr, F0_curve, N, s, noise,
             int(seed) & (2 ** 64 - 1), int(utt_offset), B, T, out, ws, nb)
        return out if in_dev.type == "cuda" else out.to(in_dev)


class F0NEngine(_Engine):
    """HIP forward of ProsodyPredictor.F0Ntrain's conv stacks (reference models.py:451-461)."""

    def __init__(self, module, dtype="fp32"):
        super().__init__(module, dtype)
        self.d_hid, self.style_dim = module.d_hid, module.style_dim
        self.model = NativeModel(KIND_F0N, [module.d_hid, module.style_dim], module)
        self.model.pack(dtype)

    def forward_nlc(self, x, s):
        """x: shared-LSTM output [B, T, d_hid] (batch_first); s [B, style_dim] -> (F0, N) [B, 2T]."""
        dev = self.model.device
        in_dev = x.device
        x, s = _dev_f32(x, dev), _dev_f32(s, dev)
        B, T, D = x.shape
        if D != self.d_hid or tuple(s.shape) != (B, self.style_dim):
            raise ValueError(f"F0Ntrain inputs: x {tuple(x.shape)}, s {tuple(s.shape)}")
        if T < 2:  # as the reference's InstanceNorm1d on a single frame
            raise ValueError(f"F0Ntrain inputs: need at least 2 frames, got {T}")
        F0 = torch.empty(B, 2 * T, dtype=torch.float32, device=dev)
        Nn = torch.empty(B, 2 * T, dtype=torch.float32, device=dev)
        ws, nb = self.model.workspace(self.dtype, B, T)
        call("stts_f0n_fwd", self.model.h, DTYPES[self.dtype], x, s, B, T, F0, Nn, ws, nb)
        if in_dev.type != "cuda":
            return F0.to(in_dev), Nn.to(in_dev)
        return F0, Nn


class StyleEngine(_Engine):
    """HIP forward of models.py StyleEncoder (reference models.py:145-150)."""

    def __init__(self, module, dtype="fp32"):
        super().__init__(module, dtype)
        d_in = module.shared[0].cout
        self.style_dim = module.style_dim
        max_conv = max(d for _, d in module.dims)
        self.model = NativeModel(KIND_STYLE, [d_in, module.style_dim, max_conv], module)
        self.model.pack(dtype)

    def forward(self, mel):
        dev = self.model.device
        in_dev = mel.device
        mel = _dev_f32(mel, dev)
        B, one, M, T = mel.shape
        if one != 1 or M != 80:
            raise ValueError(f"mel must be [B, 1, 80, T], got {tuple(mel.shape)}")
        out = torch.empty(B, self.style_dim, dtype=torch.float32, device=dev)
        ws, nb = self.model.workspace(self.dtype, B, T)
        call("stts_style_fwd", self.model.h, DTYPES[self.dtype], mel, B, T, out, ws, nb)
        return out if in_dev.type == "cuda" else out.to(in_dev)


class PitchEngine(_Engine):
    """HIP forward of Modules/JDC/model.py JDCNet (reference :102-137, eval mode).  The plan binds the BatchNorm
    running statistics like any other parameter, so the packed folds go stale (stale()) when one changes."""

    def __init__(self, module, dtype="fp32"):
        super().__init__(module, dtype)
        self.num_class = module.num_class
        self.model = NativeModel(KIND_PITCH, [module.num_class], module)
        self.model.pack(dtype)

    def forward(self, mel, features=True):
        """mel [B, 1, 80, T] -> (f0 [B, T, num_class], GAN_feature [B, 256, 10, T], poolblock_out [B, 256, T, 2]);
        features=False passes null pointers for the two feature maps (they come back as None)."""
        from . import prosody
        dev = self.model.device
        in_dev = mel.device
        mel = _dev_f32(mel, dev)
        if mel.dim() != 4 or mel.shape[1] != 1 or mel.shape[2] != 80 or mel.shape[0] < 1 or mel.shape[3] < 1:
            raise ValueError(f"mel must be [B, 1, 80, T], got {tuple(mel.shape)}")
        B, _, _, T = mel.shape
        f0 = torch.empty(B, T, self.num_class, dtype=torch.float32, device=dev)
        gan = torch.empty(B, 256, 10, T, dtype=torch.float32, device=dev) if features else None
        pool = torch.empty(B, 256, T, 2, dtype=torch.float32, device=dev) if features else None
        ws, nb = self.model.workspace(self.dtype, B, T)
        call("stts_pitch_fwd", self.model.h, DTYPES[self.dtype], mel, B, T, f0, gan, pool, ws, nb)
        # the cooperative BiLSTM recurrence's time-out word, checked with the other BiLSTM launches' words
        off = query("stts_pitch_error_offset", self.model.h, DTYPES[self.dtype], B, T)
        if len(prosody._PENDING) >= 64:
            prosody.check_pending()
        prosody._PENDING.append((f"JDCNet bilstm_classifier B={B} T={T}", ws[off:off + 4].view(torch.int32).clone()))
        if in_dev.type != "cuda":
            f0, gan, pool = (t.to(in_dev) if t is not None else None for t in (f0, gan, pool))
        return f0, gan, pool


class AlignerEngine(_Engine):
    """HIP forward of Modules/ASR/models.py ASRCNN (reference :37-48, eval mode): the conv stack on the conv engines,
    the S2S decoder's recurrence as one persistent launch."""

    def __init__(self, module, dtype="fp32"):
        super().__init__(module, dtype)
        if dtype == "bf16":
            raise ValueError("ASRCNN: dtype must be fp32 or bf16x3 (GroupNorm and the recurrence are fp32)")
        self.n_token = module.n_token
        self.model = NativeModel(KIND_ALIGNER, module.cfg, module)
        self.model.pack(dtype)

    def forward(self, mel, pad_mask=None, tokens=None, unk_mask=None, ctc=True, s2s=True, attn=True, feature=False):
        """mel [B, 80, T] -> (ctc [B, L, n_token], s2s_logit [B, Tt + 1, n_token], attn [B, Tt + 1, L], feature
        [B, 128, L]); an output that is switched off, or that needs tokens when there are none, is None (a null
        pointer to the library)."""
        dev = self.model.device
        mel = _dev_f32(mel, dev)
        if mel.dim() != 3 or mel.shape[1] != 80 or mel.shape[0] < 1 or mel.shape[2] < 1:
            raise ValueError(f"mel must be [B, 80, T], got {tuple(mel.shape)}")
        B, _, T = mel.shape
        L = (T + 1) // 2
        as_bytes = lambda t: t.to(device=dev).ne(0).to(torch.uint8).contiguous()  # noqa: E731
        if pad_mask is not None:
            if tuple(pad_mask.shape) != (B, L):
                raise ValueError(f"src_key_padding_mask must be [B, {L}], got {tuple(pad_mask.shape)}")
            pad_mask = as_bytes(pad_mask)
        Tt = 0
        if tokens is not None:
            if tokens.dim() != 2 or tokens.shape[0] != B or tokens.shape[1] < 1:
                raise ValueError(f"text_input must be [B, T_text >= 1], got {tuple(tokens.shape)}")
            Tt = tokens.shape[1]
            tokens = tokens.to(device=dev, dtype=torch.int32).contiguous()
            if unk_mask is not None:
                if tuple(unk_mask.shape) != (B, Tt):
                    raise ValueError(f"unk_mask must be [B, {Tt}], got {tuple(unk_mask.shape)}")
                unk_mask = as_bytes(unk_mask)
        new = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)  # noqa: E731
        o_ctc = new(B, L, self.n_token) if ctc else None
        o_s2s = new(B, Tt + 1, self.n_token) if s2s and Tt else None
        o_attn = new(B, Tt + 1, L) if attn and Tt else None
        o_feat = new(B, 128, L) if feature else None
        dt = DTYPES[self.dtype]
        nb = query("stts_aligner_workspace_bytes", self.model.h, dt, B, T, Tt)
        ws = self.model._ws.get(self.dtype)
        if ws is None or ws.numel() < nb:
            self.model._ws[self.dtype] = ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)
        call("stts_aligner_fwd", self.model.h, dt, mel, pad_mask, tokens, unk_mask if Tt else None, B, T, Tt, o_ctc,
             o_s2s, o_attn, o_feat, ws, nb)
        return o_ctc, o_s2s, o_attn, o_feat


def log_norm(x, mean=-4, std=4, dim=2):
    """utils.py:48-53 on the HIP path (stts_log_norm), for the call train.py:262 makes: x [B, 1, n_mels, T] with
    dim = 2 (the mel axis) -> [B, 1, T] = log(|| exp(x * std + mean) ||_2)."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[1] != 1 or dim != 2:
        raise NotImplementedError("log_norm: the HIP path serves train.py:262's call only, x [B, 1, n_mels, T] with "
                                  f"dim=2 (got {tuple(x.shape) if isinstance(x, torch.Tensor) else type(x)}, dim={dim})")
    _require_device()
    dev = x.device if x.is_cuda else torch.device("cuda", torch.cuda.current_device())
    in_dev = x.device
    m = _dev_f32(x, dev)
    B, _, M, T = m.shape
    out = torch.empty(B, 1, T, dtype=torch.float32, device=dev)
    if B and T:
        call("stts_log_norm", m, B, M, T, mean, std, out)
    return out if in_dev.type == "cuda" else out.to(in_dev)


MPD_CH = (1, 32, 128, 512, 1024, 1024, 1)


def mpd_lengths(T: int, p: int):
    """Frame counts of DiscriminatorP(p)'s 6 feature maps over T samples (plan.cpp mpd_lengths)."""
    L = [(T + p - 1) // p]
    for _ in range(4):
        L.append((L[-1] + 4 - 5) // 3 + 1)
    L.append(L[-1])
    return L


class _DiscEngine(_Engine):
    """What the two discriminator engines share: the GAN losses of the last forward."""

    LOSSES = None  # the subclass names its loss entry point

    def gan_losses(self):
        """losses.py:97-128 feature_loss, generator_loss[0], discriminator_loss[0] of the last
        forward, whose batch was B real then B generated waveforms: device float64 tensor [3]."""
        out, B2, T = self.last
        if B2 % 2:
            raise ValueError("the last forward's batch is not real + generated halves")
        nb = query("stts_gan_losses_scratch_bytes", self.model.h)
        scratch = torch.empty(nb // 8, dtype=torch.float64, device=out.device)
        loss = torch.empty(3, dtype=torch.float64, device=out.device)
        call(self.LOSSES, self.model.h, B2 // 2, T, out, scratch, nb, loss)
        return loss


class MPDEngine(_DiscEngine):
    """HIP forward of Modules/discriminators.py MultiPeriodDiscriminator's DiscriminatorP stacks
    (reference :108-129): one batch of waveforms [B, 1, T] -> per period (scores [B, L*p], fmaps)."""

    LOSSES = "stts_mpd_losses"

    def __init__(self, module, dtype="fp32"):
        super().__init__(module, dtype)
        self.periods = [d.period for d in module.discriminators]
        self.model = NativeModel(KIND_MPD, [len(self.periods), *self.periods], module)
        self.model.pack(dtype)

    def forward(self, x):
        dev = self.model.device
        in_dev = x.device
        w = _dev_f32(x, dev)
        if w.dim() != 3 or w.shape[1] != 1:
            raise ValueError(f"waveform must be [B, 1, T], got {tuple(w.shape)}")
        B, _, T = w.shape
        for p in self.periods:
            if (-T) % p >= T:
                raise ValueError(f"T = {T} too short for the period-{p} reflect pad")
        n = query("stts_mpd_out_elems", self.model.h, B, T)
        out = torch.empty(n, dtype=torch.float32, device=dev)
        ws, nb = self.model.workspace(self.dtype, B, T)
        call("stts_mpd_fwd", self.model.h, DTYPES[self.dtype], w, B, T, out, n, ws, nb)
        self.last = (out, B, T)
        res, off = [], 0
        for p in self.periods:
            L = mpd_lengths(T, p)
            fmaps = []
            for j in range(6):
                C, Lj = MPD_CH[j + 1], L[j + 1] if j < 5 else L[5]
                k = B * p * Lj * C
                # frames [B*p][L][C] -> the reference's [B, C, L, p] (a permuted view)
                f = out[off:off + k].view(B, p, Lj, C).permute(0, 3, 2, 1)
                fmaps.append(f if in_dev.type == "cuda" else f.to(in_dev))
                off += k
            score = torch.flatten(fmaps[-1], 1, -1)  # discriminators.py:129
            res.append((score, fmaps))
        return res


def msd_geometry(T, n_fft, hop):
    """SpecDiscriminator map sizes over T samples (plan.cpp:msd_geom): H frames, widths W[0..5]."""
    H = 1 + T // hop
    W = [n_fft // 2 + 1] * 2
    for _ in range(3):
        W.append((W[-1] - 1) // 2 + 1)
    W.append(W[-1])
    return H, W


class MSDEngine(_DiscEngine):
    """HIP forward of Modules/discriminators.py MultiResSpecDiscriminator's SpecDiscriminator stacks
    (reference :47-63): one batch of waveforms [B, 1, T] -> per resolution (scores [B, H*W], fmaps)."""

    LOSSES = "stts_msd_losses"

    def __init__(self, module, dtype="fp32"):
        super().__init__(module, dtype)
        self.res = [(d.fft_size, d.shift_size, d.win_length) for d in module.discriminators]
        cfg = [len(self.res)] + [v for r in self.res for v in r]
        self.model = NativeModel(KIND_MSD, cfg, module)
        self.model.pack(dtype)

    def forward(self, x):
        dev = self.model.device
        in_dev = x.device
        w = _dev_f32(x, dev)
        if w.dim() == 3:
            if w.shape[1] != 1:
                raise ValueError(f"waveform must be [B, 1, T] or [B, T], got {tuple(w.shape)}")
            w = w[:, 0]
        B, T = w.shape
        for n_fft, _, _ in self.res:
            if T <= n_fft // 2:  # torch.stft's reflect pad
                raise ValueError(f"T = {T} too short for n_fft {n_fft}")
        w = w.contiguous()
        n = query("stts_msd_out_elems", self.model.h, B, T)
        out = torch.empty(n, dtype=torch.float32, device=dev)
        ws, nb = self.model.workspace(self.dtype, B, T)
        call("stts_msd_fwd", self.model.h, DTYPES[self.dtype], w, B, T, out, n, ws, nb)
        self.last = (out, B, T)
        res, off = [], 0
        for n_fft, hop, _ in self.res:
            H, W = msd_geometry(T, n_fft, hop)
            fmaps = []
            for j in range(6):
                C, Wj = (32, W[j + 1]) if j < 5 else (1, W[5])
                k = B * H * Wj * C
                f = out[off:off + k].view(B, H, Wj, C).permute(0, 3, 1, 2)  # -> [B, C, H, W] (a view)
                fmaps.append(f if in_dev.type == "cuda" else f.to(in_dev))
                off += k
            res.append((torch.flatten(fmaps[-1], 1, -1), fmaps))  # discriminators.py:63
        return res


N_MELS, MEL_HOP, MEL_NFFT = 80, 300, 2048


def wave_preprocess_batch(wave):
    """HIP log-mel of B equal-length waves: wave [B, L] (any device) -> device [B, 80, 1 + L // 300]
    (reference inference.py:43-49 per row).  L must exceed 1024, as the reference's reflect
    padding requires."""
    _require_device()
    dev = torch.device("cuda", torch.cuda.current_device())
    w = _dev_f32(wave, dev)
    if w.dim() != 2:
        raise ValueError(f"wave must be [B, L], got {tuple(w.shape)}")
    B, L = w.shape
    if L <= MEL_NFFT // 2:
        raise ValueError(f"wave of {L} samples: the reflect padding of n_fft {MEL_NFFT} needs more than "
                         f"{MEL_NFFT // 2}")
    F = int(lib().stts_mel_frames(L))
    out = torch.empty(B, N_MELS, F, dtype=torch.float32, device=dev)
    call("stts_wave_preprocess", w, B, L, L, out, ws=("stts_mel_workspace_bytes",))
    return out


def profile_enable(on: bool = True):
    call("stts_profile_enable", 1 if on else 0)


def profile_read():
    t, n, f, b = ctypes.c_double(), c_ll(), ctypes.c_double(), ctypes.c_double()
    call("stts_profile_read", ctypes.byref(t), ctypes.byref(n), ctypes.byref(f), ctypes.byref(b))
    return {"ms": t.value, "launches": n.value, "flops": f.value, "bytes": b.value}


ENGINE_KERNELS = ("conv1d_igemm_kernel", "k_resconv", "k_bigconv", None, "k_conv_post",
                  "k_pwgemm", "k_ressplit", "k_bigconv2[SP]")  # engine ids 0..7 (3: retired, no launch records it)


def profile_launches():
    """Per-launch records of the timed region: dicts with the GEMM shape, the kernel the launch
    was routed to, ms, flops, bytes."""
    out = []
    n = profile_read()["launches"]
    shape, v = (ctypes.c_int * 8)(), (ctypes.c_double * 3)()
    for i in range(n):
        call("stts_profile_launch", i, shape, v)
        out.append({"B": shape[0], "rows": shape[1], "N": shape[2], "Cin": shape[3], "taps": shape[4],
                    "dil": shape[5], "Lout": shape[6], "res_acc": shape[7] & 3,
                    "kernel": ENGINE_KERNELS[(shape[7] >> 4) & 7], "ms": v[0], "flops": v[1], "bytes": v[2]})
    return out
