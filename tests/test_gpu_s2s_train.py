"""Training the aligner's S2S decoder on the device: asr.ASRS2S.forward (stts_s2s_fwd_train / stts_s2s_bwd),
losses.s2s_loss and losses.mono_loss against the reference's fixtures (tests/golden/make_golden_s2s_train.py) and a
plain-torch restatement (tests/s2s_ref.py) run in fp64 on the device."""
import ctypes
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN, fill_module
from s2s_ref import KEYS, s2s_forward
from stts2_mi355x import synth
from test_gpu_train_pred import _check_fixture

pytestmark = pytest.mark.gpu
N_TOKEN, EMB, D = 35, 256, 128
CASES = ("A", "B", "Bdrop", "C", "D")


def _net():
    from stts2_mi355x.asr import ASRCNN
    return fill_module(ASRCNN(), "asr.").asr_s2s.cuda()


def _case(name):
    fx = np.load(os.path.join(GOLDEN, f"s2s_train_{name}.npz"))
    B, L, Tt = int(fx["B"]), int(fx["L"]), int(fx["Tt"])
    mem = np.stack([synth.normal(f"s2s:mem:{b}:{L}", (L, D)) for b in range(B)])
    mask = None
    if fx["mem_lens"][0] >= 0:
        mask = torch.from_numpy(np.arange(L)[None, :] >= fx["mem_lens"][:, None]).cuda()
    probes = [torch.from_numpy(synth.normal(f"s2s:probe:{k}:{B}:{L}:{Tt}", shp)).cuda() for k, shp in
              (("h", (B, Tt + 1, D)), ("l", (B, Tt + 1, N_TOKEN)), ("a", (B, Tt + 1, L)))]
    return fx, torch.from_numpy(mem).cuda(), mask, torch.from_numpy(fx["tokens"]).cuda(), \
        torch.from_numpy(fx["unk_mask"]), probes


def _run(net, mem, mask, tok, unk, probes, train=False):
    from stts2_mi355x import training as Tr
    net.train(train)
    net.zero_grad(set_to_none=True)
    m = mem.clone().requires_grad_(True)
    Tr.set_dropout_masks(synth.dropout_mask if train else None)
    try:
        out = net(m, mask, tok, unk_mask=unk)
    finally:
        Tr.set_dropout_masks(None)
    sum((o * p).sum() for o, p in zip(out, probes)).backward()
    grads = {k: p.grad for k, p in net.named_parameters()}
    grads["dmemory"] = m.grad
    return out, grads


def _fwd_bar(out, ref, ref_err, what):
    err = float((out.detach().double().cpu() - torch.as_tensor(ref).double().cpu()).abs().max())
    scale = max(1.0, float(torch.as_tensor(ref).abs().max()))
    print(f"{what}: {err / scale:.2e} (fp32 reference vs fp64 {ref_err:.2e})")
    assert err / scale <= max(1e-4, 4.0 * ref_err), (what, err, ref_err)


@pytest.mark.parametrize("name", CASES)
def test_parity_with_reference(name):
    fx, mem, mask, tok, unk, probes = _case(name)
    out, grads = _run(_net(), mem, mask, tok, unk, probes, train=bool(fx["train"]))
    for k, o in zip(("hidden", "logit", "attn"), out):
        _fwd_bar(o, fx[k], float(fx[k + "_fp32_vs_fp64"]), f"{name} {k}")
    _check_fixture(grads, fx, f"s2s {name}")
    if mask is not None:  # masked frames: exactly 0 in the weights and in dmemory
        assert float(out[2][mask[:, None, :].expand_as(out[2])].abs().max()) == 0.0
        assert float(grads["dmemory"][mask].abs().max()) == 0.0


def test_against_torch_restatement():
    """B = 1, L = 300, T_text = 24: a longer feedback chain and three conv tiles; truth = the restatement in fp64 on
    the device under torch autograd, the "reference's error" = its own fp32 run."""
    B, L, Tt = 1, 300, 24
    net = _net()
    mem = torch.from_numpy(synth.normal("s2s:mem:long", (B, L, D))).cuda()
    tok = torch.from_numpy(4 + (synth.hash_u01("s2s:tok:long", Tt) * (N_TOKEN - 4)).astype(np.int64))[None].cuda()
    unk = torch.zeros(B, Tt, dtype=torch.bool)
    unk[0, 5] = True
    probes = [torch.from_numpy(synth.normal(f"s2s:probe:long:{k}", shp)).cuda() for k, shp in
              (("h", (B, Tt + 1, D)), ("l", (B, Tt + 1, N_TOKEN)), ("a", (B, Tt + 1, L)))]
    out, grads = _run(net, mem, None, tok, unk, probes)
    res = {}
    for dt in (torch.float64, torch.float32):
        ps = [p.detach().to(dt).requires_grad_(True) for _, p in net.named_parameters()]
        m = mem.to(dt).requires_grad_(True)
        o = s2s_forward(ps, m, None, tok, unk.cuda())
        sum((a * p.to(dt)).sum() for a, p in zip(o, probes)).backward()
        res[dt] = ([a.detach() for a in o], {**{k: p.grad for k, p in zip(KEYS, ps)}, "dmemory": m.grad})
    (o64, g64), (o32, g32) = res[torch.float64], res[torch.float32]
    for k, a, r64, r32 in zip(("hidden", "logit", "attn"), out, o64, o32):
        _fwd_bar(a, r64, float((r32.double() - r64).abs().max()), f"restatement {k}")
    gm = max(float(g.abs().max()) for g in g64.values())
    for k in g64:
        scale = max(float(g64[k].abs().max()), 1e-3 * gm)
        eo = float((grads[k].double() - g64[k]).abs().max()) / scale
        er = float((g32[k].double() - g64[k]).abs().max()) / scale
        print(f"restatement {k}: {eo:.2e} (fp32 torch {er:.2e})")
        assert eo <= max(2.0 * er, 1e-4), (k, eo, er)


def test_forward_bits_match_aligner_forward():
    """ASRS2S in eval mode on ASRCNN's own feature returns the logits and alignments of ASRCNN.forward bit for bit."""
    from stts2_mi355x.asr import ASRCNN
    fx = np.load(os.path.join(GOLDEN, "aligner_B3_T41_Tt9.npz"))
    net = fill_module(ASRCNN(n_token=178, token_embedding_dim=512), "asr.").eval().cuda()
    mel = np.stack([synth.normal(f"aligner:mel:{b}:41", (80, 41)) for b in range(3)])
    for b, n in enumerate(fx["mel_lens"]):
        mel[b, :, n:] = 0.0
    mel, tok, unk = torch.from_numpy(mel).cuda(), torch.from_numpy(fx["tokens"]).cuda(), torch.from_numpy(fx["unk_mask"])
    L = 21
    mask = (torch.arange(L)[None, :] + 1 > (torch.from_numpy(fx["mel_lens"]) // 2)[:, None]).cuda()
    _, s2s, attn = net(mel, mask, tok, unk_mask=unk)
    memory = net.get_feature(mel).transpose(1, 2).contiguous()
    with torch.no_grad():
        _, logit, align = net.asr_s2s(memory, mask, tok, unk_mask=unk)
    assert torch.equal(logit, s2s) and torch.equal(align, attn)


def test_deterministic_and_batch_invariant():
    fx, mem, mask, tok, unk, probes = _case("C")
    net = _net()
    _, g1 = _run(net, mem, mask, tok, unk, probes)
    g1 = {k: v.clone() for k, v in g1.items()}
    _, g2 = _run(net, mem, mask, tok, unk, probes)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    for b in range(mem.shape[0]):
        _, gb = _run(net, mem[b:b + 1], mask[b:b + 1], tok[b:b + 1], unk[b:b + 1], [p[b:b + 1] for p in probes])
        assert torch.equal(gb["dmemory"][0], g1["dmemory"][b]), b


def _raw(B, L, Tt, skip=(), ws_cut=0, with_dmem=True):
    """stts_s2s_fwd_train + stts_s2s_bwd called directly; returns (rc, dmemory, grads)."""
    from stts2_mi355x.engine import lib, query
    net = _net()
    ps = [p.detach().contiguous() for _, p in net.named_parameters()]
    mem = torch.from_numpy(synth.normal(f"s2s:raw:{L}", (B, L, D))).cuda()
    tok = torch.full((B, Tt), 7, dtype=torch.int32, device="cuda")
    hid = torch.empty(B, Tt + 1, D, device="cuda")
    logit = torch.empty(B, Tt + 1, N_TOKEN, device="cuda")
    attn = torch.empty(B, Tt + 1, L, device="cuda")
    arr = (ctypes.c_void_p * 14)(*[p.data_ptr() for p in ps])
    Lq = min(L, 4096)  # (the size queries refuse what the entries refuse)
    sv = torch.empty(query("stts_s2s_save_bytes", B, Lq, Tt), dtype=torch.uint8, device="cuda")
    wf = torch.empty(query("stts_s2s_fwd_train_workspace_bytes", B, Lq, Tt, N_TOKEN, EMB), dtype=torch.uint8,
                     device="cuda")
    wb = torch.empty(query("stts_s2s_bwd_workspace_bytes", B, Lq, Tt, N_TOKEN, EMB), dtype=torch.uint8, device="cuda")
    rc = lib().stts_s2s_fwd_train(mem.data_ptr(), None, tok.data_ptr(), None, arr, B, L, Tt, N_TOKEN, EMB, None,
                                  hid.data_ptr(), logit.data_ptr(), attn.data_ptr(), sv.data_ptr(), wf.data_ptr(),
                                  wf.numel(), None)
    if rc != 0:
        return rc, None, None
    grads = [None if i in skip else torch.empty_like(p) for i, p in enumerate(ps)]
    garr = (ctypes.c_void_p * 14)(*[None if g is None else g.data_ptr() for g in grads])
    dmem = torch.empty_like(mem) if with_dmem else None
    dl = torch.from_numpy(synth.normal("s2s:raw:dl", (B, Tt + 1, N_TOKEN))).cuda()
    da = torch.from_numpy(synth.normal("s2s:raw:da", (B, Tt + 1, L))).cuda()
    rc = lib().stts_s2s_bwd(mem.data_ptr(), None, tok.data_ptr(), None, arr, B, L, Tt, N_TOKEN, EMB, None,
                            hid.data_ptr(), attn.data_ptr(), sv.data_ptr(), None, dl.data_ptr(), da.data_ptr(),
                            None if dmem is None else dmem.data_ptr(), garr, wb.data_ptr(), wb.numel() - ws_cut, None)
    torch.cuda.synchronize()
    return rc, dmem, grads


def test_null_gradient_pointers_leave_the_others_bitwise():
    rc, dmem, full = _raw(2, 9, 3)
    assert rc == 0
    skip = (0, 3, 6, 8, 13)
    rc, dmem2, part = _raw(2, 9, 3, skip=skip)
    assert rc == 0 and torch.equal(dmem, dmem2)
    for i, (a, b) in enumerate(zip(full, part)):
        assert (b is None) if i in skip else torch.equal(a, b), i
    rc, none, part = _raw(2, 9, 3, with_dmem=False)
    assert rc == 0 and none is None and all(torch.equal(a, b) for a, b in zip(full, part))


def test_refusals_by_return_code():
    from stts2_mi355x.asr import ASRCNN  # noqa: F401
    from stts2_mi355x.engine import lib
    assert lib().stts_s2s_bwd_workspace_bytes(1, 4097, 1, N_TOKEN, EMB) == -1  # STTS_EINVAL
    rc, _, _ = _raw(1, 4097, 1)
    assert rc == -1
    rc, _, _ = _raw(1, 5, 2, ws_cut=256)
    assert rc == -4  # STTS_EWORKSPACE
    net = _net()
    with pytest.raises(IndexError):
        net(torch.zeros(1, 4, D, device="cuda"), None, torch.tensor([[4, N_TOKEN]]))
    with pytest.raises(IndexError):
        net(torch.zeros(1, 4, D, device="cuda"), None, torch.tensor([[-1, 4]]))


def test_losses_match_train_py():
    """train.py:301-306 written in torch (fp64) on a ragged batch with lengths (9, 6, 7)."""
    import torch.nn.functional as F
    from stts2_mi355x import losses
    B, T, L = 3, 9, 21
    ln = torch.tensor([9, 6, 7])
    pred = torch.from_numpy(synth.normal("s2s:loss:pred", (B, T, N_TOKEN), 2.0)).cuda().requires_grad_(True)
    texts = torch.from_numpy((synth.hash_u01("s2s:loss:tok", B * T) * N_TOKEN).astype(np.int64).reshape(B, T)).cuda()
    attn = torch.softmax(torch.from_numpy(synth.normal("s2s:loss:attn", (B, T, L))).cuda(), -1).requires_grad_(True)
    mono = (torch.from_numpy(synth.hash_u01("s2s:loss:mono", B * T * L).reshape(B, T, L)) > 0.9).float().cuda()
    with torch.no_grad():
        attn[0, 0, :3] = mono[0, 0, :3]  # exact ties: sign(0) = 0
    ls, lm = losses.s2s_loss(pred, texts, ln), losses.mono_loss(attn, mono)
    (0.7 * ls + 1.3 * lm).backward()
    p64, a64 = pred.detach().double().requires_grad_(True), attn.detach().double().requires_grad_(True)
    rs = 0
    for _p, _t, _l in zip(p64, texts, ln):
        rs = rs + F.cross_entropy(_p[:_l], _t[:_l])
    rs = rs / B
    rm = F.l1_loss(a64, mono.double()) * 10
    (0.7 * rs + 1.3 * rm).backward()
    for what, a, r in (("loss_s2s", ls, rs), ("loss_mono", lm, rm)):
        rel = abs(float(a) - float(r)) / abs(float(r))
        print(what, float(a), float(r), rel)
        assert rel <= 1e-5
    for what, g, r in (("d loss_s2s", pred.grad, p64.grad), ("d loss_mono", attn.grad, a64.grad)):
        rel = float((g.double() - r).abs().max() / r.abs().max())
        print(what, rel)
        assert rel <= 1e-5
    with pytest.raises(IndexError):
        losses.s2s_loss(pred, texts + N_TOKEN, ln)


def test_one_adamw_step_lowers_the_loss():
    from stts2_mi355x import losses, optim
    from stts2_mi355x import training as Tr
    fx, mem, mask, tok, unk, _ = _case("C")
    net = _net().train()
    before = [p.detach().clone() for p in net.parameters()]
    opt = optim.AdamW(list(net.parameters()), lr=1e-3)
    ln = torch.from_numpy(fx["text_lens"])
    mono = torch.zeros(3, 10, 21, device="cuda")
    for t in range(10):
        mono[:, t, min(2 * t, 20)] = 1.0

    def loss():
        Tr.set_dropout_masks(synth.dropout_mask)
        try:
            _, logit, attn = net(mem, mask, tok, unk_mask=unk)
        finally:
            Tr.set_dropout_masks(None)
        return losses.s2s_loss(logit[:, 1:], tok, ln) + losses.mono_loss(attn, mono)

    l0 = loss()
    l0.backward()
    opt.step()
    assert all(not torch.equal(a, p.detach()) for a, p in zip(before, net.parameters()))
    with torch.no_grad():
        l1 = loss()
    print("loss", float(l0), "->", float(l1))
    assert float(l1) < float(l0)
