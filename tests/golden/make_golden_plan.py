"""Golden fixtures of the decoder plans' host side (csrc/plan.cpp decoder_forward / vocos_forward), recorded from a
built libstts2.so of the commit BEFORE a change to that code (STTS_LIB names it), never from the changed tree:

    STTS_LIB=<parent build>/libstts2.so PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_plan.py
    STTS_LIB=<parent build>/libstts2.so PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_plan.py launches

plan_workspace.json (no GPU): stts_workspace_bytes, i.e. the dry run's allocations and statistics, of every decoder
kind x dtype x B x T below at the default options, and of each kind at B = 2, T = 16 with the side streams off and
with the noise stream alone.  The batch sizes straddle the split-K scratch (B <= 4), STTS_OPT_BRANCHES (8),
STTS_OPT_NBRANCH (64) and the statistics slots (B <= 4, B <= 16).

plan_launches.json (`launches`, on the MI355X): the integer fields of engine.profile_launches() (every key but ms,
flops and bytes: the GEMM shape, res / acc flags and the engine) of one tiny forward per LAUNCH_CASES entry, in
launch order.  (PLAN_LAUNCHES_OUT: another path to write that file to.)
"""
from __future__ import annotations

import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, os.path.join(ROOT, "styletts2-lite_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, _p)
os.environ.pop("STTS_OPTS", None)  # lib() applies it on load

KINDS = ("hifigan", "istftnet", "vocos")
BATCHES = (1, 4, 8, 9, 16, 64, 65)
FRAMES = (4, 16, 40)
SIDE_OPTS = ((0, 0), (0, 64))  # (STTS_OPT_BRANCHES, STTS_OPT_NBRANCH) at B = 2, T = 16, beside the defaults (8, 64)
VOCOS_CFG = [512, 128, 1536, 8, 1200, 300]  # test_vocos_cpu.make_vocos()
# (kind, dtype, B, T): both forks; the noise fork alone; no forks (split accuracy mode); istftnet; vocos
LAUNCH_CASES = (("hifigan", "fp32", 1, 4), ("hifigan", "bf16", 12, 4), ("hifigan", "bf16x3", 1, 4),
                ("istftnet", "fp32", 2, 4), ("vocos", "fp32", 1, 4))
FLOAT_KEYS = ("ms", "flops", "bytes")


def plan_cfg(kind):
    """The C-ABI config of the decoder helpers.make_decoder(kind) / test_vocos_cpu.make_vocos() builds."""
    from helpers import HIFI_CFG, ISTFT_CFG
    if kind == "vocos":
        return list(VOCOS_CFG)
    g = ISTFT_CFG if kind == "istftnet" else HIFI_CFG
    cfg = [512, 128, g["upsample_initial_channel"], len(g["upsample_rates"]), *g["upsample_rates"],
           *g["upsample_kernel_sizes"], len(g["resblock_kernel_sizes"]), *g["resblock_kernel_sizes"],
           *[d for ds in g["resblock_dilation_sizes"] for d in ds]]
    return cfg + ([g["gen_istft_n_fft"], g["gen_istft_hop_size"]] if kind == "istftnet" else [])


def workspace_cases():
    """[kind, dtype, B, T, branches, nbranch] of every recorded dry run, in the fixture's order."""
    rows = [[k, dt, B, T, 8, 64] for k in KINDS for dt in (0, 1, 2) for B in BATCHES for T in FRAMES]
    return rows + [[k, dt, 2, 16, br, nbr] for k in KINDS for dt in (0, 1, 2) for br, nbr in SIDE_OPTS]


def workspace_bytes(E, cases):
    """stts_workspace_bytes of each case (one plan per kind; the options restored afterwards)."""
    L = E.lib()
    plans = {}
    for k in KINDS:
        cfg = plan_cfg(k)
        plans[k] = ctypes.c_void_p()
        kind = {"hifigan": E.KIND_HIFIGAN, "istftnet": E.KIND_ISTFTNET, "vocos": E.KIND_VOCOS}[k]
        assert L.stts_model_create(kind, (ctypes.c_int * len(cfg))(*cfg), len(cfg), ctypes.byref(plans[k])) == 0
    try:
        out = []
        for k, dt, B, T, br, nbr in cases:
            E.set_option(E.OPT_BRANCHES, br)
            E.set_option(E.OPT_NBRANCH, nbr)
            out.append(int(L.stts_workspace_bytes(plans[k], dt, B, T)))
        return out
    finally:
        E.reset_options()
        for h in plans.values():
            L.stts_model_destroy(h)


def launch_list(E, kind, dtype, B, T):
    """The integer fields of every conv launch of one forward, in launch order (needs the GPU)."""
    import torch
    from helpers import decoder_case, make_decoder
    from stts2_mi355x import synth
    if kind == "vocos":
        from test_vocos_cpu import make_vocos
        dec = make_vocos().cuda()
        args, kw = [torch.from_numpy(a).cuda() for a in synth.decoder_inputs(B, T, tag="vocos")], {}
    else:
        dec = make_decoder(kind)[0].cuda()
        *args, nz = [t.cuda() for t in decoder_case(B, T)]
        kw = {"noise": nz}
    try:
        E.profile_enable(True)
        with torch.no_grad():
            dec(*args, dtype=dtype, **kw)
        torch.cuda.synchronize()
        return [{key: v for key, v in r.items() if key not in FLOAT_KEYS} for r in E.profile_launches()]
    finally:
        E.profile_enable(False)


def _dump(path, head, rows):
    with open(path, "w") as f:  # one line per row
        f.write("{\n" + "".join(f" {json.dumps(k)}: {json.dumps(v)},\n" for k, v in head.items()))
        f.write(' "rows": [\n' + ",\n".join("  " + json.dumps(r) for r in rows) + "\n ]\n}\n")
    print(path, os.path.getsize(path))


def main():
    from stts2_mi355x import engine as E
    assert os.environ.get("STTS_LIB"), "record from the parent commit's build: set STTS_LIB"
    if sys.argv[1:] == ["launches"]:
        rows, keys = [], None
        for case in LAUNCH_CASES:
            recs = launch_list(E, *case)
            keys = keys or list(recs[0])
            rows += [["/".join(str(v) for v in case), *[r[k] for k in keys]] for r in recs]
        out = os.environ.get("PLAN_LAUNCHES_OUT") or os.path.join(HERE, "plan_launches.json")
        _dump(out, {"keys": ["case", *keys]}, rows)
    else:
        cases = workspace_cases()
        rows = [[*c, nb] for c, nb in zip(cases, workspace_bytes(E, cases))]
        _dump(os.path.join(HERE, "plan_workspace.json"),
              {"configs": {k: plan_cfg(k) for k in KINDS},
               "keys": ["kind", "dtype", "B", "T", "branches", "nbranch", "bytes"]}, rows)


if __name__ == "__main__":
    main()
