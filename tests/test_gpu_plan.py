"""The decoder plans issue the recorded launch list: tests/golden/plan_launches.json (make_golden_plan.py, recorded on
the MI355X from the build before decoder_forward was split into parts) holds, for one tiny forward per case, the
integer fields of every conv launch (GEMM shape, dilation, output rows, residual / running-sum flags, the kernel it
was routed to) in launch order.  The side streams are on where the defaults turn them on: hifigan fp32 B = 1 forks
the resblocks and the noise branches, hifigan bf16 B = 12 the noise branches alone, hifigan bf16x3 (the split
accuracy mode) and vocos nothing, istftnet fp32 B = 2 both.  Which stream a launch went to is not in the record:
the bitwise fork-against-one-stream tests (test_gpu_branches.py) and the graph replay (test_gpu_graph.py) hold that."""
import json
import os

import pytest
import torch

from helpers import GOLDEN, decoder_case, make_decoder

pytestmark = pytest.mark.gpu

CASES = [("hifigan", "fp32", 1, 4), ("hifigan", "bf16", 12, 4), ("hifigan", "bf16x3", 1, 4),
         ("istftnet", "fp32", 2, 4), ("vocos", "fp32", 1, 4)]


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "plan_launches.json")) as f:
        rec = json.load(f)
    assert rec["keys"] == ["case", "B", "rows", "N", "Cin", "taps", "dil", "Lout", "res_acc", "kernel"]
    by_case = {}
    for case, *row in rec["rows"]:
        by_case.setdefault(case, []).append(row)
    assert list(by_case) == ["/".join(str(v) for v in c) for c in CASES]
    return rec["keys"][1:], by_case


@pytest.mark.parametrize("kind,dtype,B,T", CASES)
def test_launch_list_is_the_recorded_one(recorded, kind, dtype, B, T):
    from stts2_mi355x import engine as E, synth
    keys, by_case = recorded
    want = by_case[f"{kind}/{dtype}/{B}/{T}"]
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
        got = [[r[k] for k in keys] for r in E.profile_launches()]
    finally:
        E.profile_enable(False)
    print(f"{kind} {dtype} B={B} T={T}: {len(got)} launches, recorded {len(want)}")
    assert len(want) > 20
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"launch {i}: {dict(zip(keys, g))}, recorded {dict(zip(keys, w))}"
    assert len(got) == len(want)
