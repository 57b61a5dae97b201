"""CPU tests of the C-ABI library: it loads, exports every symbol include/*.h declares, the ctypes
signature table (stts2_mi355x/abi.py) and engine's constants agree with those headers, and its model
plans name exactly the reference state-dict keys (no GPU compute here)."""
import ctypes
import glob
import json
import os
import re
import subprocess
import sys

import pytest
import torch

from helpers import HIFI_CFG, ISTFT_CFG
from stts2_mi355x import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    out = set()
    for h in sorted(glob.glob(os.path.join(ROOT, "include", "*.h"))):
        src = re.sub(r"/\*.*?\*/", "", open(h).read(), flags=re.S)
        out |= set(re.findall(r"\b(stts_[a-z0-9_]+)\s*\(", src))
    return sorted(out)


def _headers():
    """{header name: its text with the comments stripped}."""
    return {os.path.basename(h): re.sub(r"/\*.*?\*/", "", open(h).read(), flags=re.S)
            for h in sorted(glob.glob(os.path.join(ROOT, "include", "*.h")))}


# the classes a C parameter or return type reduces to; anything with a '*' is a pointer
_C_SCALARS = {"int": "int", "long long": "long long", "unsigned long long": "unsigned long long", "float": "float",
              "double": "double"}


def _c_class(decl, what, is_param):
    """Class of one C declaration (`const float* x`, `long long ws_bytes`, a bare return type): raises on anything
    that is not a pointer, one of _C_SCALARS or a void return, so that no prototype goes by unchecked."""
    words = decl.replace("*", " * ").split()
    if "*" in words:
        return "pointer"
    words = [w for w in words if w != "const"]
    for n in (3, 2, 1):  # the longest type name first: `unsigned long long`, then `long long`, then `int`
        t = " ".join(words[:n])
        if t in _C_SCALARS and len(words) == n + (1 if is_param else 0):  # a parameter carries its name
            return _C_SCALARS[t]
    if not is_param and words == ["void"]:
        return "void"
    raise AssertionError(f"{what}: cannot classify {decl!r}")


def header_prototypes():
    """{name: ([argument classes], return class)} of every `<type> stts_name(<params>);` in include/*.h."""
    protos = {}
    for fname, src in _headers().items():
        src = re.sub(r"^\s*#.*$", "", src, flags=re.M)  # preprocessor lines
        for ret, name, params in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(stts_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src):
            assert name not in protos, f"{fname}: {name} declared twice"
            params = params.strip()
            args = [] if params in ("", "void") else [
                _c_class(p, f"{fname}: {name} parameter {k}", True) for k, p in enumerate(params.split(","))]
            protos[name] = (args, _c_class(ret, f"{fname}: {name} return type", False))
    return protos


def _ctypes_class(t, what):
    """Class of one entry of abi.SIGNATURES, in header_prototypes()' terms."""
    scalars = {ctypes.c_int: "int", ctypes.c_longlong: "long long", ctypes.c_ulonglong: "unsigned long long",
               ctypes.c_float: "float", ctypes.c_double: "double", None: "void"}
    if t in scalars:
        return scalars[t]
    if t in (ctypes.c_void_p, ctypes.c_char_p) or (isinstance(t, type) and issubclass(t, ctypes._Pointer)):
        return "pointer"
    raise AssertionError(f"{what}: cannot classify {t!r}")


def test_library_exports_all_declared_symbols():
    L = E.lib()
    syms = declared_symbols()
    assert len(syms) >= 14 + 20  # stts2.h + stts2_train.h
    for s in syms:
        assert hasattr(L, s), f"libstts2.so does not export {s}"


def test_every_prototype_is_parsed():
    """The prototype parser sees every declared name (a prototype its regex misses is an error, not an omission)."""
    protos = header_prototypes()
    assert sorted(protos) == declared_symbols()
    assert len(protos) == len(declared_symbols())


def test_signature_table_names_the_declared_entry_points():
    assert set(E.SIGNATURES) - set(declared_symbols()) == set(), "bound but not declared in include/*.h"
    assert set(declared_symbols()) - set(E.SIGNATURES) == set(), "declared in include/*.h but not in abi.SIGNATURES"


def test_signature_table_matches_the_headers():
    """Argument count, the class of every argument and of the return value, header against abi.SIGNATURES."""
    protos = header_prototypes()
    bad = []
    for name, (args, res) in E.SIGNATURES.items():
        want_args, want_res = protos[name]
        got_args = [_ctypes_class(t, f"{name} argument {k}") for k, t in enumerate(args)]
        got_res = _ctypes_class(res, f"{name} restype")
        if got_args != want_args or got_res != want_res:
            bad.append(f"{name}: header ({', '.join(want_args)}) -> {want_res}; "
                       f"table ({', '.join(got_args)}) -> {got_res}")
    assert not bad, "\n".join(bad)


def test_loaded_library_carries_the_table():
    """After lib() every entry point of the table is typed on the loaded library, whichever module asks for it."""
    L = E.lib()
    for name, (args, res) in E.SIGNATURES.items():
        fn = getattr(L, name)
        assert fn.argtypes is not None and list(fn.argtypes) == list(args), name
        assert fn.restype is res, name


def _defines(prefix):
    """{NAME: int value} of every `#define <prefix>NAME <integer>` in include/*.h."""
    out = {}
    for src in _headers().values():
        for name, val in re.findall(rf"^\s*#\s*define\s+{prefix}(\w+)\s+\(?(-?\d+)\)?\s*$", src, flags=re.M):
            assert name not in out, f"{prefix}{name} defined twice"
            out[name] = int(val)
    return out


def test_constants_match_the_header():
    """engine's ABI_VERSION, OPT_* (with a default each) and KIND_* are the header's #defines, in both directions."""
    assert _defines("STTS_ABI_")["VERSION"] == E.ABI_VERSION
    opts = _defines("STTS_OPT_")
    assert opts
    for name, val in opts.items():
        assert getattr(E, "OPT_" + name, None) == val, f"STTS_OPT_{name} = {val}"
        assert val in E.OPT_DEFAULTS, f"OPT_{name} has no entry in OPT_DEFAULTS"
    for name in dir(E):
        if name.startswith("OPT_") and name != "OPT_DEFAULTS":
            assert name[4:] in opts, f"engine.{name} has no #define STTS_{name}"
    kinds = _defines("STTS_KIND_")
    assert kinds
    for name, val in kinds.items():
        assert getattr(E, "KIND_" + name, None) == val, f"STTS_KIND_{name} = {val}"
    for name in dir(E):
        if name.startswith("KIND_"):
            assert name[5:] in kinds, f"engine.{name} has no #define STTS_{name}"


def _plan(kind, cfg):
    L = E.lib()
    arr = (ctypes.c_int * len(cfg))(*cfg)
    h = ctypes.c_void_p()
    rc = L.stts_model_create(kind, arr, len(cfg), ctypes.byref(h))
    return rc, h


def _dec_cfg(module, ist):
    g = module.generator
    cfg = [module.dim_in, module.style_dim, g.upsample_initial_channel, len(g.upsample_rates), *g.upsample_rates,
           *g.upsample_kernel_sizes, len(g.resblock_kernel_sizes), *g.resblock_kernel_sizes,
           *[d for ds in g.resblock_dilation_sizes for d in ds]]
    return cfg + ([g.gen_istft_n_fft, g.gen_istft_hop_size] if ist else [])


@pytest.mark.parametrize("kind", ["hifigan", "istftnet"])
def test_decoder_plan_names_match_state_dict(kind):
    from stts2_mi355x.hifigan import Decoder as H
    from stts2_mi355x.istftnet import Decoder as I
    ist = kind == "istftnet"
    mod = (I if ist else H)(dim_in=512, style_dim=128, dim_out=80, **(ISTFT_CFG if ist else HIFI_CFG))
    rc, h = _plan(1 if ist else 0, _dec_cfg(mod, ist))
    assert rc == 0
    L = E.lib()
    sd = mod.state_dict()
    names = [L.stts_param_name(h, i).decode() for i in range(L.stts_param_count(h))]
    assert sorted(names) == sorted(sd.keys())
    for i, n in enumerate(names):
        assert L.stts_param_numel(h, i) == sd[n].numel(), n
    assert L.stts_packed_bytes(h, 1) > 0 and L.stts_packed_bytes(h, 0) > L.stts_packed_bytes(h, 1)
    ws = L.stts_workspace_bytes(h, 1, 32, 400)
    assert 0 < ws < 8 << 30  # B=32 x 10 s in bf16 fits a few GB of the 288 GB HBM
    # forward without packed weights / params must fail loudly, not compute
    rc = L.stts_decoder_fwd(h, 0, None, None, None, None, None, 0, 0, 1, 4, None, None, 0, None)
    assert rc < 0
    L.stts_model_destroy(h)


def test_f0n_plan_names_match_state_dict():
    from stts2_mi355x.models import ProsodyPredictor
    pp = ProsodyPredictor(style_dim=128, d_hid=512, nlayers=3, max_dur=50, dropout=0.2)
    rc, h = _plan(2, [512, 128])
    assert rc == 0
    L = E.lib()
    sd = pp.state_dict()
    names = [L.stts_param_name(h, i).decode() for i in range(L.stts_param_count(h))]
    assert set(names) <= set(sd.keys())
    assert {n for n in sd if n.startswith(("F0.", "N.", "F0_proj", "N_proj"))} == set(names)
    L.stts_model_destroy(h)


def test_bad_configs_rejected():
    assert _plan(0, [512, 128, 512, 4, 10, 5, 3])[0] < 0       # truncated
    assert _plan(0, [512, 128, 256, 1, 2, 4, 1, 3, 1, 3, 5])[0] < 0  # init channel must be 512
    assert _plan(7, [1])[0] < 0                                 # unknown kind
    assert _plan(2, [511, 128])[0] < 0                          # odd d_hid


def test_error_strings():
    L = E.lib()
    for code in (0, -1, -2, -3, -4, -5):
        assert L.stts_error_string(code)


def test_product_path_refuses_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from helpers import make_decoder
    dec, _ = make_decoder("hifigan")
    with pytest.raises(RuntimeError):
        dec(torch.zeros(1, 512, 4), torch.zeros(1, 8), torch.zeros(1, 8), torch.zeros(1, 128))


def test_style_plan_names_match_state_dict():
    from stts2_mi355x.models import StyleEncoder
    se = StyleEncoder(dim_in=64, style_dim=128, max_conv_dim=512)
    rc, h = _plan(3, [64, 128, 512])
    assert rc == 0
    L = E.lib()
    sd = se.state_dict()
    names = [L.stts_param_name(h, i).decode() for i in range(L.stts_param_count(h))]
    assert sorted(names) == sorted(sd.keys())
    for i, n in enumerate(names):
        assert L.stts_param_numel(h, i) == sd[n].numel(), n
    assert L.stts_workspace_bytes(h, 0, 1, 241) > 0
    assert L.stts_workspace_bytes(h, 0, 1, 48) < 0  # 5x5 valid conv needs T >= 65 (reference raises too)
    L.stts_model_destroy(h)


def test_duration_path_argument_checks():
    """The duration-path entry points validate shapes before touching the device (include/stts2.h)."""
    L = E.lib()
    assert L.stts_bilstm_workspace_bytes(2, 10, 256) == ((2 * 2 * 10 * 1024 + 2 * 256 * 1024) * 4 + 2 * 2 * 2 * 256 * 8 + 8
                                                          + 16 * 2 * 10 * 1024 * 4)  # split-K scratch (B T <= 256)
    assert L.stts_bilstm_workspace_bytes(32, 400, 256) == (2 * 32 * 400 * 1024 + 2 * 256 * 1024) * 4 + 2 * 32 * 2 * 256 * 8 + 8
    params = (ctypes.c_void_p * 8)(*([1] * 8))
    # H must be a multiple of 32 and <= 256
    assert L.stts_bilstm_fwd(1, 0, 0, 0, 1, 4, 8, None, params, 300, 1, None, None, 1, 1 << 30, None) == -1
    assert L.stts_bilstm_fwd(1, 0, 0, 0, 1, 4, 8, None, params, 24, 1, None, None, 1, 1 << 30, None) == -1
    # workspace too small
    assert L.stts_bilstm_fwd(1, 0, 0, 0, 1, 4, 8, None, params, 32, 1, None, None, 1, 16, None) == -4
    assert L.stts_row_norm(1, 0, 0, 0, 1, 1, 8, 3, 1, 1, 0, 1e-5, 0, 0.0, None, None, 0, 1, 0, 0, None) == -1
    assert L.stts_frames_gemm(1, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 0, 1, 0, 0, None, None, 1, 0, 0, 0, 1, None) == -1


def test_duration_modules_keep_reference_keys():
    """TextEncoder / ProsodyPredictor expose the reference's state-dict names (models.py:241-466)."""
    from stts2_mi355x.models import ProsodyPredictor, TextEncoder
    te = TextEncoder(channels=512, kernel_size=5, depth=3, n_symbols=178)
    keys = set(te.state_dict())
    for k in ("embedding.weight", "cnn.2.0.weight_g", "cnn.2.0.weight_v", "cnn.2.0.bias", "cnn.2.1.gamma",
              "cnn.2.1.beta", "lstm.weight_hh_l0_reverse", "lstm.bias_ih_l0"):
        assert k in keys, k
    assert len(keys) == 1 + 3 * 5 + 8
    pp = ProsodyPredictor(style_dim=128, d_hid=512, nlayers=3, max_dur=50, dropout=0.2)
    pk = set(pp.state_dict())
    for k in ("text_encoder.lstms.0.weight_ih_l0", "text_encoder.lstms.5.fc.weight", "lstm.bias_hh_l0_reverse",
              "duration_proj.linear_layer.weight", "shared.weight_hh_l0"):
        assert k in pk, k
    with pytest.raises(RuntimeError):
        te(torch.zeros(1, 4, dtype=torch.long), torch.tensor([4]))


def test_option_defaults_are_the_documented_ones():
    """engine.OPT_DEFAULTS (what tests restore) equals the library's own production defaults."""
    from stts2_mi355x import engine
    engine.reset_options()
    for k, v in engine.OPT_DEFAULTS.items():
        assert engine.get_option(k) == v, (k, engine.get_option(k), v)
    assert engine.lib().stts_get_option(999) < 0


@pytest.mark.parametrize("key", [3, 9, 26, 28])
def test_retired_option_keys_are_invalid(key):
    """The retired STTS_OPT_* keys (include/stts2.h) are neither settable nor readable: STTS_EINVAL, no launch."""
    from stts2_mi355x import engine
    L = engine.lib()
    assert key not in engine.OPT_DEFAULTS
    assert L.stts_set_option(key, 1) == -1  # STTS_EINVAL
    assert L.stts_get_option(key) == -1


def test_option_semantics_are_the_recorded_ones():
    """stts_set_option / stts_get_option accept, normalise and refuse exactly as the library did before the options
    moved into one table: tests/golden/option_semantics.json (make_golden_options.py) holds, for every key live
    then and every probe value, [rc of set, get afterwards], the key at its initial value before each probe.  A key
    recorded there and no longer live must be retired (STTS_EINVAL both ways), as must the keys recorded invalid."""
    L = E.lib()
    with open(os.path.join(ROOT, "tests", "golden", "option_semantics.json")) as f:
        rec = json.load(f)
    probes = rec["probes"]
    assert probes == [-2, -1, 0, 1, 2, 3, 4, 5, 6, 7, 64, 65, 1 << 20]
    assert len(rec["live"]) == 26 and sorted(rec["invalid"]) == sorted(["3", "9", "26", "28", "999"])
    bad = []
    try:
        for name, row in rec["live"].items():
            key = row["key"]
            assert len(row["results"]) == len(probes), name
            for v, want in zip(probes, row["results"]):
                if key in E.OPT_DEFAULTS:
                    assert L.stts_set_option(key, row["initial"]) == 0, name
                else:
                    want = [-1, -1]
                got = [L.stts_set_option(key, v), L.stts_get_option(key)]
                if got != want:
                    bad.append(f"STTS_OPT_{name} <- {v}: (rc, value) {got}, recorded {want}")
        for key, rows in rec["invalid"].items():
            for v, want in zip(probes, rows):
                assert want == [-1, -1]
                got = [L.stts_set_option(int(key), v), L.stts_get_option(int(key))]
                if got != want:
                    bad.append(f"key {key} <- {v}: (rc, value) {got}, recorded {want}")
    finally:
        E.reset_options()
    assert not bad, "\n".join(bad)


def test_fresh_library_holds_the_production_defaults():
    """The library's own initialisers equal engine's production defaults: a fresh process (no STTS_OPTS) loads the
    library, sets nothing and reads every key.  (test_option_defaults_are_the_documented_ones resets the options
    first, so it cannot see an initialiser that disagrees with engine.OPT_DEFAULTS.)  No GPU is touched."""
    code = ("import json, sys; sys.path.insert(0, sys.argv[1]); from stts2_mi355x import engine as E; L = E.lib(); "
            "print(json.dumps({str(k): L.stts_get_option(k) for k in E.OPT_DEFAULTS}))")
    env = {k: v for k, v in os.environ.items() if k != "STTS_OPTS"}
    r = subprocess.run([sys.executable, "-c", code, os.path.join(ROOT, "styletts2-lite_amd")], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = {int(k): v for k, v in json.loads(r.stdout.strip().splitlines()[-1]).items()}
    production = {k: d for _, k, d in E._OPTS}  # (OPT_DEFAULTS before any STTS_OPTS override of this process)
    assert len(production) == 26
    assert got == production, {k: (got.get(k), d) for k, d in production.items() if got.get(k) != d}


def test_decoder_workspace_bytes_are_the_recorded_ones():
    """The decoder plans' dry run (every allocation and the statistics region: the workspace layout the kernels and
    a captured graph see) sizes the workspace exactly as the library did before decoder_forward was split into
    parts: tests/golden/plan_workspace.json (make_golden_plan.py) holds stts_workspace_bytes for hifigan / istftnet /
    vocos x dtype 0, 1, 2 x B in (1, 4, 8, 9, 16, 64, 65) x T in (4, 16, 40) at the default options, and for each
    kind at B = 2, T = 16 with the side streams off and with the noise stream alone.  Dry runs: no GPU."""
    from test_vocos_cpu import make_vocos
    L = E.lib()
    with open(os.path.join(ROOT, "tests", "golden", "plan_workspace.json")) as f:
        rec = json.load(f)
    kinds = {"hifigan": E.KIND_HIFIGAN, "istftnet": E.KIND_ISTFTNET, "vocos": E.KIND_VOCOS}
    want_cases = [[k, dt, B, T, 8, 64] for k in kinds for dt in (0, 1, 2) for B in (1, 4, 8, 9, 16, 64, 65)
                  for T in (4, 16, 40)]
    want_cases += [[k, dt, 2, 16, br, nbr] for k in kinds for dt in (0, 1, 2) for br, nbr in ((0, 0), (0, 64))]
    assert [r[:6] for r in rec["rows"]] == want_cases  # the recorded cross product, whole and in order
    assert E.OPT_DEFAULTS[E.OPT_BRANCHES] == 8 and E.OPT_DEFAULTS[E.OPT_NBRANCH] == 64
    from stts2_mi355x.hifigan import Decoder as H
    from stts2_mi355x.istftnet import Decoder as I
    v = make_vocos()
    cfgs = {"hifigan": _dec_cfg(H(dim_in=512, style_dim=128, dim_out=80, **HIFI_CFG), False),
            "istftnet": _dec_cfg(I(dim_in=512, style_dim=128, dim_out=80, **ISTFT_CFG), True),
            "vocos": [v.dim_in, v.style_dim, v.generator.intermediate_dim, v.generator.num_layers, v.generator.n_fft,
                      v.generator.hop]}
    assert rec["configs"] == cfgs  # the configs helpers.make_decoder / make_vocos build
    plans = {}
    bad = []
    try:
        for k, cfg in cfgs.items():
            rc, plans[k] = _plan(kinds[k], cfg)
            assert rc == 0, k
        for k, dt, B, T, br, nbr, want in rec["rows"]:
            assert want > 0
            E.set_option(E.OPT_BRANCHES, br)
            E.set_option(E.OPT_NBRANCH, nbr)
            got = L.stts_workspace_bytes(plans[k], dt, B, T)
            if got != want:
                bad.append(f"{k} dtype {dt} B {B} T {T} BRANCHES {br} NBRANCH {nbr}: {got} bytes, recorded {want}")
    finally:
        E.reset_options()
        for h in plans.values():
            L.stts_model_destroy(h)
    assert not bad, "\n".join(bad)


def _mpd_elems(B, T, p):
    """Floats of DiscriminatorP(p)'s 6 maps over B signals of T samples, by engine's mirror of the geometry."""
    Ls = E.mpd_lengths(T, p)
    return sum(B * p * (Ls[j + 1] if j < 5 else Ls[5]) * E.MPD_CH[j + 1] for j in range(6))


def _msd_elems(B, T, n_fft, hop):
    H, W = E.msd_geometry(T, n_fft, hop)
    return sum(B * H * (W[j + 1] if j < 5 else W[5]) * (32 if j < 5 else 1) for j in range(6))


def _scratch_bytes(n):
    return 6 * n * 64 * 4 * 8  # 6 maps per discriminator x 64 partial blocks x 4 sums x sizeof(double)


def test_mpd_map_list_matches_the_python_mirror():
    """stts_mpd_out_elems and the loss scratch size (both read plan.cpp's one map list) against engine.mpd_lengths /
    MPD_CH, per period and for the five together; the (period, T) pairs stts_mpd_fwd refuses for the reflect pad
    are left out."""
    L = E.lib()
    periods, Ts = (2, 3, 5, 7, 11), (2, 3, 7, 100, 1201)
    legal = lambda p, T: T >= 2 and (-T) % p < T  # noqa: E731
    checked = 0
    for ps in [(p,) for p in periods] + [periods]:
        rc, h = _plan(E.KIND_MPD, [len(ps), *ps])
        assert rc == 0
        assert L.stts_gan_losses_scratch_bytes(h) == _scratch_bytes(len(ps))
        for B in (1, 2):
            for T in Ts:
                if all(legal(p, T) for p in ps):
                    assert L.stts_mpd_out_elems(h, B, T) == sum(_mpd_elems(B, T, p) for p in ps), (ps, B, T)
                    checked += 1
        L.stts_model_destroy(h)
    assert checked == 2 * (5 + 5 + 4 + 3 + 3 + 3)  # T = 2 is legal for periods 2, 3; T = 3 for 2, 3, 5; T >= 7 for all


def test_msd_map_list_matches_the_python_mirror():
    """stts_msd_out_elems and the loss scratch size against engine.msd_geometry, per resolution at its smallest legal
    T (n_fft / 2 + 1) and at 2,400, and for the three together at 2,400."""
    L = E.lib()
    res = ((16, 4, 16), (1024, 120, 600), (2048, 240, 1200))
    for rs in [(r,) for r in res] + [res]:
        rc, h = _plan(E.KIND_MSD, [len(rs)] + [v for r in rs for v in r])
        assert rc == 0
        assert L.stts_gan_losses_scratch_bytes(h) == _scratch_bytes(len(rs))
        for B in (1, 2):
            for T in sorted({max(r[0] for r in rs) // 2 + 1, 2400}):
                assert L.stts_msd_out_elems(h, B, T) == sum(_msd_elems(B, T, r[0], r[1]) for r in rs), (rs, B, T)
        L.stts_model_destroy(h)


@pytest.mark.parametrize("kind", [-1, 7, 9, 100])
def test_unknown_kinds_rejected(kind):
    rc, h = _plan(kind, [1])
    assert rc == -1 and not h.value  # STTS_EINVAL, no model


def test_bilstm_error_word_offset():
    """The BiLSTM error word lies inside the workspace, 8-byte aligned, before the exchange words."""
    L = E.lib()
    for B, T, H in ((1, 5, 256), (4, 37, 256), (32, 400, 256), (3, 7, 64)):
        off = L.stts_bilstm_error_offset(B, T, H)
        assert 0 < off and off % 8 == 0 and off + 8 <= L.stts_bilstm_workspace_bytes(B, T, H)
    assert L.stts_bilstm_error_offset(-1, 1, 1) < 0


# ---------------------------------------------------------------------- engine.call / engine.query
def test_stream_is_the_last_parameter_wherever_it_appears():
    """engine.call appends the current stream when the caller leaves one argument out: sound only if every prototype
    with a parameter named `stream` has it last."""
    seen = set()
    for fname, src in _headers().items():
        src = re.sub(r"^\s*#.*$", "", src, flags=re.M)
        for name, params in re.findall(r"\b(stts_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src):
            names = [re.split(r"[\s\*]+", p.strip())[-1] for p in params.split(",")]
            if "stream" in names:
                seen.add(name)
                assert names.index("stream") == len(names) - 1 and names.count("stream") == 1, f"{fname}: {name}"
                assert E.SIGNATURES[name][0][-1] is ctypes.c_void_p, name
    assert {"stts_decoder_fwd", "stts_linear_fwd", "stts_snake_bwd", "stts_adamw_step"} <= seen  # the parser sees them


def test_size_query_through_the_helper():
    assert E.query("stts_snake_workspace_bytes", 2, 3, 4) == E.lib().stts_snake_workspace_bytes(2, 3, 4) > 0


def test_invalid_size_query_raises_with_its_name():
    with pytest.raises(RuntimeError, match="stts_snake_workspace_bytes failed: .* \\(code -\\d+\\)"):
        E.query("stts_snake_workspace_bytes", 0, 3, 4)
    with pytest.raises(TypeError, match="stts_snake_workspace_bytes"):  # a query is no status: no stream to append
        E.call("stts_snake_workspace_bytes", 2, 3)


def test_call_refuses_a_wrong_argument_count_before_anything_runs():
    """Two arguments too few and one too many name the entry and both counts; they raise before the stream lookup
    (which needs a device), as does one too few for an entry that takes no stream."""
    n = len(E.SIGNATURES["stts_linear_fwd"][0])
    with pytest.raises(TypeError, match=f"stts_linear_fwd takes {n} arguments.*got {n - 2}"):
        E.call("stts_linear_fwd", *([None] * (n - 2)))
    with pytest.raises(TypeError, match=f"stts_linear_fwd takes {n} arguments.*got {n + 1}"):
        E.call("stts_linear_fwd", *([None] * (n + 1)))
    with pytest.raises(TypeError, match="stts_snake_bwd takes 11 arguments.*got 9 \\+ workspace"):
        E.call("stts_snake_bwd", *([None] * 9), ws=("stts_snake_workspace_bytes", 2, 3, 4))
    with pytest.raises(TypeError, match="stts_set_option takes 2 arguments, got 1"):
        E.call("stts_set_option", 1)


def test_call_converts_tensors_at_the_pointer_positions_only():
    """The converter of stts_linear_fwd against a stub in the library function's place: data_ptr() ints at exactly
    the c_void_p positions of its signature, None untouched (ctypes' NULL), the three ints and an explicit stream as
    given; the stub's status raises in check()'s format."""
    args_t = E.SIGNATURES["stts_linear_fwd"][0]
    assert [t is ctypes.c_void_p for t in args_t] == [True, True, True, False, False, False, True, True]
    got = []

    def stub(*a):
        got.append(a)
        return 0

    s, W, h = torch.zeros(2, 3), torch.zeros(4, 3), torch.zeros(2, 4)
    cached = E._ENTRIES.get("stts_linear_fwd")
    E._bind("stts_linear_fwd", stub)((s, W, None, 2, 3, 4, h, 0))
    assert got == [(s.data_ptr(), W.data_ptr(), None, 2, 3, 4, h.data_ptr(), 0)]
    assert all(type(v) is int for v in got[0] if v is not None)
    assert E._ENTRIES.get("stts_linear_fwd") is cached  # a stub's converter does not replace the library's
    with pytest.raises(RuntimeError, match="^stts_linear_fwd failed: .* \\(code -1\\)$"):
        E._bind("stts_linear_fwd", lambda *a: -1)((s, W, None, 2, 3, 4, h, 0))
