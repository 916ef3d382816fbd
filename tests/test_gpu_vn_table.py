"""FX_TERM_VNCLASS in the loss term table (csrc/vnloss.hip + vloss.hip) and the verb/noun model's
one-table loss phase (models/vn_vloss.py) (GPU).

Kernel level: tables of VNCLASS (and FX_TERM_ATTN) terms through fx_loss_terms_fwd / _bwd against the
float64 restatement of tests/test_gpu_vn_loss.py (loss.py:8-18, 209-277; blocks_SepVerbNoun.py:189-224,
271-283) on the materialised tables.  Bounds as there: scalars rtol 2e-5,
gradients 2e-5 x (1 + max|ref|).
Model level: ``tiny_vn`` with the table on and off, and the ``tiny_vn_o2m`` fixture (o2m matching with
more than 64 matched columns) against the reference's values.
"""
import numpy as np
import pytest
import torch

import paramgen as pg
from factmx import functional as fxf
from factmx import native as nx
from factmx.models.termtable import TermTable, _Pack
from helpers import load_fixture, tiny_meta, cfg_from_meta, tiny_inputs, check_grad
from test_gpu_verbnoun import _mapping, _close
from test_gpu_vn_loss import loss_case, seg_case, _r

pytestmark = pytest.mark.gpu
DEV = "cuda"
UP = 1.7          # upstream factor of the cases' gradients


def i32(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.int32).to(DEV).contiguous()


def run_table(specs):
    """One term table of ``specs`` (dicts: VNCLASS terms ``x, m, null, y, w, c_ce, c_sm[, rs, re, D]``, ATTN
    terms ``L, axis, ka, kgs, kge, ksw, rs, re, c_ce``): out = [UP * sum of the terms, each term], the
    backward of out[0].  Returns (out, [gradient of each term's logits])."""
    n = len(specs)
    inputs = [(s["x"] if "x" in s else s["L"]) for s in specs]
    coef = np.zeros((1 + n, n), dtype=np.float32)
    coef[0, :] = UP
    coef[1:, :] = np.eye(n)
    tt = TermTable(_Pack(), DEV, inputs, coef, nvn=n)       # (every VNCLASS term its own mapping)
    tt.gflat.fill_(float("nan"))
    for i, s in enumerate(specs):
        c_ce, c_sm = s["c_ce"], s.get("c_sm", 0.0)
        if "x" in s:
            x, m, null = s["x"], s["m"], s["null"]
            C = m.num_verbs + m.num_nouns + 2 * null
            t = tt.add(nx.TERM_VNCLASS, x.shape[0], C, x.data_ptr(), x.stride(0), 1, x, 0, x.shape[1], 1, c_ce, c_sm)
            t.vn, t.vn_host = tt.vn(i, m, null)
            t.w = s["w"].data_ptr()
            if s.get("y") is not None:
                t.y = s["y"].data_ptr()
            if "rs" in s:
                t.rs, t.re, t.D = s["rs"].data_ptr(), s["re"].data_ptr(), s["D"]
        else:
            L = s["L"]
            K = len(s["ka"])
            t = tt.add(nx.TERM_ATTN, L.shape[0], L.shape[1], L.data_ptr(), L.stride(0), L.stride(1), L, 0,
                       L.shape[1], 1, c_ce, c_sm, K)
            t.axis, t.K = s["axis"], K
            t.rs, t.re = s["rs"].data_ptr(), s["re"].data_ptr()
            t.ka, t.kgs, t.kge, t.ksw = (s[k].data_ptr() for k in ("ka", "kgs", "kge", "ksw"))
    tt.lay_out()
    tt.send()
    out, loss = tt.launch(keep=specs)
    grads = torch.autograd.grad(loss, inputs)
    torch.cuda.synchronize()
    return out.detach(), [g.clone() for g in grads]


def vn_spec(case, m, null, seg=False):
    x = case["base"].float().to(DEV).requires_grad_(True)
    s = dict(x=x, m=m, null=null, y=i32(case["y"]), w=case["w"].float().to(DEV), c_ce=case["c_ce"],
             c_sm=case.get("c_sm", 0.0))
    if seg:
        s.update(rs=i32(case["st"]), re=i32(case["en"]), D=len(case["y"]))
    return s


def check_vn(out_i, grad, case, what):
    print(f"{what}: out {out_i.item():.8g} ref {case['out'].item():.8g}")
    np.testing.assert_allclose(out_i.item(), case["out"].item(), rtol=2e-5, err_msg=what)
    _close(grad, case["grad"], what=what + " dclogit")
    assert not bool(torch.isnan(grad).any())


# ---------------------------------------------------------------------------
# VNCLASS terms
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("action,smooth", [(False, False), (False, True), (True, False)],
                         ids=["hard", "hard_smooth", "token_null"])
@pytest.mark.parametrize("V,N,A", [(5, 7, 12), (98, 301, 4000)])
@pytest.mark.parametrize("R", [1, 3, 300])
def test_vnclass_hard_targets(R, V, N, A, action, smooth):
    """R = 300 > FX_LOSS_NB: workgroups take several rows."""
    assert 300 > nx.LOSS_NB
    vids, nids = _mapping(V, N, A, seed=A)
    m = fxf.VerbNounMap(vids, nids)
    case = loss_case(R, V, N, vids, nids, action, smooth)
    out, grads = run_table([vn_spec(case, m, 1 if action else 0)])
    check_vn(out[1], grads[0], case, f"R={R} A={A} action={action} smooth={smooth}")
    np.testing.assert_allclose(out[0].item(), UP * case["out"].item(), rtol=2e-5)


SEG_LENS = {1: [371], 3: [1, 300, 5], 300: [1, 300, 7, 40] + [2] * 296}


@pytest.mark.parametrize("V,N,A", [(5, 7, 12), (98, 301, 4000)])
@pytest.mark.parametrize("R", [1, 3, 300])
def test_vnclass_segment_targets(R, V, N, A):
    """Segment rows over frame labels; one segment is longer than a workgroup (300, 371 > 256 frames)."""
    lens = SEG_LENS[R]
    assert len(lens) == R and max(lens) > 256
    vids, nids = _mapping(V, N, A, seed=A)
    m = fxf.VerbNounMap(vids, nids)
    case = seg_case(V, N, vids, nids, lens, seed=R)
    out, grads = run_table([vn_spec(case, m, 0, seg=True)])
    check_vn(out[1], grads[0], case, f"segments R={R} A={A}")


# ---------------------------------------------------------------------------
# a mixed table: two VNCLASS widths and an ATTN term with repeated token columns
# ---------------------------------------------------------------------------

def attn_case(axis, seed=0):
    """cross_attn_loss_tdu (loss.py:224-244) in float64: S = 40 TDU rows over T = 300 frames, G = K = 70
    ground-truth segments matched to 16 tokens with repeats (as o2m pairs them)."""
    T, S, G, Q = 300, 40, 70, 16
    rng = np.random.default_rng(seed)

    def cut(parts):
        b = np.sort(rng.choice(np.arange(1, T), parts - 1, replace=False))
        lens = np.diff(np.concatenate([[0], b, [T]]))
        en = np.cumsum(lens) - 1
        return en - lens + 1, en
    st, en = cut(S)
    gs, ge = cut(G)
    ka = rng.integers(0, Q, G)
    ka[:4] = [3, 3, 7, 3]
    ksw = rng.uniform(0.5, 1.5, G)
    base = _r(S, Q, scale=2.0, seed=seed + 5)
    L = base.clone().requires_grad_(True)
    tdu_of = np.repeat(np.arange(S), en - st + 1)
    gt_of = np.repeat(np.arange(G), ge - gs + 1)
    onehot = torch.nn.functional.one_hot(torch.from_numpy(gt_of), G).double()
    z = torch.zeros(S, G, dtype=torch.float64).index_add_(0, torch.from_numpy(tdu_of), onehot)
    z = z / torch.from_numpy((en - st + 1).astype(np.float64))[:, None]
    lp = torch.log_softmax(L[:, torch.from_numpy(ka)], dim=axis)          # dim - 1 of the reference call
    out = (-lp * z * torch.from_numpy(ksw)).sum() / z.sum()
    (UP * out).backward()
    spec = dict(L=base.float().to(DEV).requires_grad_(True), axis=axis, ka=i32(ka), kgs=i32(gs), kge=i32(ge),
                ksw=torch.from_numpy(ksw).float().to(DEV), rs=i32(st), re=i32(en), c_ce=1.0 / S)
    return spec, out.detach(), L.grad


@pytest.mark.parametrize("axis", [0, 1])
def test_mixed_table_and_bitwise_repeat(axis):
    v1, n1 = _mapping(5, 7, 12)
    v2, n2 = _mapping(98, 301, 4000, seed=4000)
    m1, m2 = fxf.VerbNounMap(v1, n1), fxf.VerbNounMap(v2, n2)
    small = loss_case(67, 5, 7, v1, n1, True, False, seed=3)
    big = loss_case(67, 98, 301, v2, n2, False, True, seed=4)
    runs = []
    for _ in range(2):
        aspec, aout, agrad = attn_case(axis, seed=axis)
        assert len(aspec["ka"]) == 70 and len(set(aspec["ka"].tolist())) < 70
        out, grads = run_table([vn_spec(small, m1, 1), aspec, vn_spec(big, m2, 0)])
        runs.append((out, grads))
    out, grads = runs[0]
    check_vn(out[1], grads[0], small, "narrow VNCLASS term")
    check_vn(out[3], grads[2], big, "wide VNCLASS term with the smooth term")
    print(f"ATTN axis {axis} K=70: out {out[2].item():.8g} ref {aout.item():.8g}")
    np.testing.assert_allclose(out[2].item(), aout.item(), rtol=2e-5)
    _close(grads[1], agrad, what="dL")
    total = UP * (small["out"] + aout + big["out"]).item()
    np.testing.assert_allclose(out[0].item(), total, rtol=2e-5)
    assert torch.equal(runs[0][0], runs[1][0])
    for a, b in zip(runs[0][1], runs[1][1]):
        assert torch.equal(a, b)


def test_table_refuses_vnclass_rows_narrower_than_the_mapping():
    vids, nids = _mapping(5, 7, 12)
    m = fxf.VerbNounMap(vids, nids)
    case = loss_case(3, 5, 7, vids, nids, False, False)
    spec = vn_spec(case, m, 0)
    spec["m"] = fxf.VerbNounMap(vids[:-1] + [5], nids)        # a sixth verb: the rows are too narrow
    with pytest.raises((nx.FactmxNativeError, ValueError)):
        run_table([spec])


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------

def _vn_step(fixture, table, monkeypatch, poison=False, second_video=False):
    from factmx.models import blocks_SepVerbNoun as vn
    from factmx.models import vn_vloss
    from factmx.models.loss import MatchCriterion
    monkeypatch.setattr(vn, "FUSED_LOSS", True)
    monkeypatch.setattr(vn_vloss, "FUSED_TABLE", table)
    fx = load_fixture(fixture)
    meta = tiny_meta(fx)
    cfg = cfg_from_meta(meta)
    vn.set_verb_noun_ids(fx["vids"].tolist(), fx["nids"].tolist())
    net = vn.FACT(cfg, meta["D"], meta["V"], meta["N"])
    with torch.no_grad():
        for n, p in net.named_parameters():
            p.copy_(torch.from_numpy(pg.param_value(n, p.shape, meta["seed"])))
    net.mcriterion = MatchCriterion(cfg, meta["C"], [])
    net = net.to(DEV).train()
    captured = {}
    orig = net.mcriterion.match

    def match_spy(*a, **k):
        captured["m"] = orig(*a, **k)
        return captured["m"]
    net.mcriterion.match = match_spy
    if poison:
        def boom(*a, **k):
            raise AssertionError("the per-term path ran with the table on")
        monkeypatch.setattr(fxf, "vn_class_loss", boom)
        monkeypatch.setattr(MatchCriterion, "cross_attn_loss_tdu", boom)
    feats, label, _ = tiny_inputs(meta)
    seqs, labels = [torch.from_numpy(feats).float().to(DEV)], [torch.from_numpy(label).to(DEV)]
    if second_video:                   # the first video's table must outlive the second video's forward
        seqs.append(torch.from_numpy(feats[::-1][:131].copy()).float().to(DEV))
        labels.append(torch.from_numpy(label[::-1][:131].copy()).to(DEV))
    total, saves = net(seqs, labels, compute_loss=True)
    total.backward()
    torch.cuda.synchronize()
    return fx, meta, net, total, saves, captured["m"]


def _against_fixture(fx, net, total, saves, match):
    np.testing.assert_allclose(total.item(), fx["loss"][0], rtol=2e-5)
    np.testing.assert_array_equal(saves[0]["pred"], fx["pred"])
    np.testing.assert_array_equal(match[0].numpy(), fx["match_a"])
    np.testing.assert_array_equal(match[1].numpy(), fx["match_s"])
    for n, prm in net.named_parameters():
        assert prm.grad is not None, n
        rms = float(fx[f"gradsum/{n}"][1]) / np.sqrt(prm.grad.numel())
        check_grad(fx, "", n, prm.grad.cpu(), rtol=2e-3, atol=2e-3 * rms + 1e-6)


def test_tiny_vn_table_on_vs_off(monkeypatch):
    fx, meta, net, total, saves, match = _vn_step("tiny_vn", True, monkeypatch, poison=True)
    monkeypatch.undo()
    _, _, net0, total0, saves0, match0 = _vn_step("tiny_vn", False, monkeypatch)
    print(f"tiny_vn loss: table {total.item():.8g} per-term {total0.item():.8g} reference {fx['loss'][0]:.8g}")
    np.testing.assert_allclose(total.item(), total0.item(), rtol=2e-5)
    np.testing.assert_array_equal(saves[0]["pred"], saves0[0]["pred"])
    assert torch.equal(match[0], match0[0]) and torch.equal(match[1], match0[1])
    assert match[0].dtype == torch.int64 and match[0].device.type == "cpu"
    assert len(net.loss_list) == len(net.block_list)
    for a, b in zip(net.loss_list, net0.loss_list):
        np.testing.assert_allclose(a.item(), b.item(), rtol=2e-5)
    np.testing.assert_allclose(sum(v.item() for v in net.loss_list) / len(net.loss_list), total.item(), rtol=2e-5)
    for (n, p), (_, p0) in zip(net.named_parameters(), net0.named_parameters()):
        rms = float(fx[f"gradsum/{n}"][1]) / np.sqrt(p.grad.numel())
        np.testing.assert_allclose(p.grad.cpu().numpy(), p0.grad.cpu().numpy(), rtol=2e-3, atol=2e-3 * rms + 1e-6,
                                   err_msg=n)
    _against_fixture(fx, net, total, saves, match)
    _against_fixture(fx, net0, total0, saves0, match0)
    # the frame-level attention stayed lazy on the table path and resolves to the gather of the segment rows
    blk = net.block_list[-1]
    assert not torch.is_tensor(blk.__dict__["_lz_a2f_attn"])
    assert torch.equal(blk.a2f_attn, blk.tdu.attn_seg2frame(blk.a2f_seg_attn))
    assert torch.equal(blk.a2f_attn, net0.block_list[-1].a2f_attn)


@pytest.mark.parametrize("table", [True, False], ids=["table", "per_term"])
def test_tiny_vn_o2m_against_the_reference(table, monkeypatch):
    """o2m matching, K = 72 > 64 matched columns with repeated tokens, T = 300, block IUU."""
    fx, meta, net, total, saves, match = _vn_step("tiny_vn_o2m", table, monkeypatch, poison=table)
    K = len(fx["match_a"])
    assert meta["Loss"]["match"] == "o2m" and K > 64 and len(set(fx["match_a"].tolist())) < K
    print(f"tiny_vn_o2m loss: {'table' if table else 'per-term'} {total.item():.8g} reference {fx['loss'][0]:.8g}")
    _against_fixture(fx, net, total, saves, match)
    assert len(net.loss_list) == 3


def test_two_videos_in_one_step_table_on_vs_off(monkeypatch):
    """Both videos' tables are built before the one backward: each keeps what its backward reads."""
    fx, meta, net, total, saves, _ = _vn_step("tiny_vn", True, monkeypatch, poison=True, second_video=True)
    monkeypatch.undo()
    _, _, net0, total0, saves0, _ = _vn_step("tiny_vn", False, monkeypatch, second_video=True)
    print(f"two videos: table {total.item():.8g} per-term {total0.item():.8g}")
    np.testing.assert_allclose(total.item(), total0.item(), rtol=2e-5)
    for a, b in zip(saves, saves0):
        np.testing.assert_array_equal(a["pred"], b["pred"])
        np.testing.assert_allclose(a["loss"]["loss"], b["loss"]["loss"], rtol=2e-5)
    for (n, p), (_, p0) in zip(net.named_parameters(), net0.named_parameters()):
        g0 = p0.grad.cpu().numpy()
        rms = float(np.sqrt((g0 * g0).mean()))
        np.testing.assert_allclose(p.grad.cpu().numpy(), g0, rtol=2e-3, atol=2e-3 * rms + 1e-6, err_msg=n)
