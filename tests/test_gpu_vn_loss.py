"""The factorised verb/noun loss and prediction kernels (csrc/vnloss.hip) and the model path built on
them (GPU).

Every op is checked against a float64 torch restatement of the reference's lines (loss.py:8-18,
246-277; blocks_SepVerbNoun.py:189-224, 271-283, 323-342) on the materialised tables.

Bounds: the scalar to rtol 2e-5, ``dclogit`` to 2e-5 x (1 + max|ref|) (``_close`` of
tests/test_gpu_verbnoun.py).  The same restatement run in float32 on the CPU sits at most 2.2e-7
(relative) from the float64 scalar and 6.9e-7 x (1 + max|ref|) from the float64 gradient over the
cases below -- under one third of the bounds, which therefore stand.
"""
import numpy as np
import pytest
import torch

import paramgen as pg
from factmx import functional as fxf
from helpers import load_fixture, tiny_meta, cfg_from_meta, tiny_inputs, check_grad
from test_gpu_verbnoun import _mapping, _close, SEG_VIDS, SEG_NIDS, SEG_V, SEG_N

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _r(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


# ---------------------------------------------------------------------------
# float64 restatement
# ---------------------------------------------------------------------------

def ref_logp(cl, vids, nids, n1, action):
    lv, ln = torch.log_softmax(cl[:, :n1], -1), torch.log_softmax(cl[:, n1:], -1)
    a = lv[:, vids] + ln[:, nids]
    if action:
        a = torch.cat([a, (lv[:, -1] + ln[:, -1]).unsqueeze(-1)], -1)
    return a


def ref_terms(lp, w, c_ce, c_sm, target=None, frame_label=None, st=None, en=None):
    """c_ce * sum of the CE terms + c_sm * sum of the smooth terms of a materialised table."""
    C = lp.shape[1]
    out = lp.new_zeros(())
    if target is not None:                       # frame_loss / action_token_loss: one-hot rows
        onehot = torch.nn.functional.one_hot(target, C).to(lp.dtype)
        out = out + c_ce * (-lp * onehot * w[:C]).sum()
    if frame_label is not None:                  # frame_loss_tdu: the zoomed one-hots
        onehot = torch.nn.functional.one_hot(frame_label, C).to(lp.dtype)
        seg = torch.zeros(len(frame_label), dtype=torch.int64)
        for s, (a, b) in enumerate(zip(st.tolist(), en.tolist())):
            seg[a:b + 1] = s
        z = torch.zeros(lp.shape[0], C, dtype=lp.dtype).index_add_(0, seg, onehot)
        z = z / (en - st + 1).to(lp.dtype)[:, None]
        out = out + c_ce * (-lp * z * w[:C]).sum()
    if c_sm:
        d = lp[1:] - lp[:-1]
        out = out + c_sm * torch.clamp(d * d, min=0, max=16).sum()
    return out


def smooth_branches(lp):
    """(fraction of clamped entries, closest | |d| - 4 |) of the smooth term of a table."""
    d = (lp[1:] - lp[:-1]).abs()
    return float((d > 4).double().mean()), float((d - 4).abs().min())


def loss_case(R, V, N, vids, nids, action, smooth, pad=0, seed=0, dtype=torch.float64):
    """Inputs of one hard-target case and its restatement in ``dtype`` (scalar, gradient, table)."""
    k = 1 if action else 0
    n1, n2, A = V + k, N + k, len(vids)
    base = _r(R, n1 + n2 + pad, scale=2.0, seed=seed + R)
    rng = np.random.default_rng(seed + 11 * R)
    y = torch.from_numpy(rng.integers(0, A, R))
    y[0] = A - 1
    if action:                                   # unmatched tokens target the null column
        y[rng.random(R) < 0.4] = A
        y[-1] = A
    w = torch.from_numpy(rng.uniform(0.5, 1.5, A + k))
    c_ce = 0.25 / R
    c_sm = 5.0 / ((R - 1) * A) if (smooth and R > 1) else 0.0
    br = base.to(dtype).clone().requires_grad_(True)
    lp = ref_logp(br[:, pad // 2:pad // 2 + n1 + n2], vids, nids, n1, action)
    out = ref_terms(lp, w.to(dtype), c_ce, c_sm, target=y)
    (1.7 * out).backward()
    return dict(base=base, y=y, w=w, c_ce=c_ce, c_sm=c_sm, n=n1 + n2, pad=pad, out=out.detach(), grad=br.grad,
                lp=lp.detach())


def run_hard(case, m, action):
    bd = case["base"].float().to(DEV).requires_grad_(True)
    p = case["pad"]
    cl = bd[:, p // 2:p // 2 + case["n"]]
    out = fxf.vn_class_loss(cl, m, case["w"].float().to(DEV), target=case["y"].to(DEV), c_ce=case["c_ce"],
                            c_sm=case["c_sm"], action=action)
    assert out.dim() == 0
    (1.7 * out).backward()
    return out, bd.grad, cl


def check_hard(R, V, N, vids, nids, action, smooth, pad=0, seed=0):
    m = fxf.VerbNounMap(vids, nids)
    case = loss_case(R, V, N, vids, nids, action, smooth, pad=pad, seed=seed)
    if case["c_sm"]:
        frac, gap = smooth_branches(case["lp"])
        print(f"smooth R={R} A={len(vids)}: clamped {frac:.3f}, closest | |d| - 4 | = {gap:.2e}")
        assert gap > 1e-5, "a difference sits on the clamp's edge"
        if R * len(vids) > 100:
            assert 0.0 < frac < 1.0, "both branches of the clamp must occur"
    out, grad, cl = run_hard(case, m, action)
    print(f"R={R} A={len(vids)} action={action} smooth={smooth}: out {out.item():.8g} ref {case['out'].item():.8g}")
    np.testing.assert_allclose(out.item(), case["out"].item(), rtol=2e-5)
    _close(grad, case["grad"], what="dclogit")
    return cl


# ---------------------------------------------------------------------------
# hard targets (+ smooth term)
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("action,smooth", [(False, False), (False, True), (True, False)])
@pytest.mark.parametrize("V,N,A", [(5, 7, 12), (98, 301, 4000)])
@pytest.mark.parametrize("R", [1, 3, 67])
def test_vn_loss_hard_targets(R, V, N, A, action, smooth):
    vids, nids = _mapping(V, N, A, seed=A)
    check_hard(R, V, N, vids, nids, action, smooth)


@pytest.mark.parametrize("action,smooth", [(False, True), (True, False)])
def test_vn_loss_empty_and_crowded_bins_strided(action, smooth):
    """Verb 3 owns no action, verb 2 owns 300; the logits are a column slice (ld > n1 + n2)."""
    V, N, A = 6, 9, 700
    rng = np.random.default_rng(3)
    vids = np.concatenate([np.full(300, 2), rng.choice([0, 1, 4, 5], A - 300)])
    rng.shuffle(vids)
    vids[-1] = 5
    nids = rng.integers(0, N, A)
    nids[0] = N - 1
    cl = check_hard(5, V, N, vids.tolist(), nids.tolist(), action, smooth, pad=10)
    assert cl.stride(0) > cl.shape[1]


def test_vn_loss_no_rows_and_refusals():
    vids, nids = _mapping(5, 7, 12)
    m = fxf.VerbNounMap(vids, nids)
    w = torch.ones(12, device=DEV)
    cl = torch.zeros(0, 12, device=DEV, requires_grad=True)
    out = fxf.vn_class_loss(cl, m, w, target=torch.zeros(0, dtype=torch.int64, device=DEV), c_ce=1.0, c_sm=1.0)
    out.backward()
    assert out.item() == 0.0 and tuple(cl.grad.shape) == (0, 12)
    with pytest.raises(ValueError):
        fxf.vn_class_loss(torch.zeros(2, 11, device=DEV), m, w, target=torch.zeros(2, dtype=torch.int64), c_ce=1.0)
    with pytest.raises(ValueError):          # a host label outside the classes is refused before any launch
        fxf.vn_class_loss(torch.zeros(2, 12, device=DEV), m, w, target=torch.tensor([0, 12]), c_ce=1.0)
    with pytest.raises(ValueError):
        fxf.vn_class_loss(torch.zeros(2, 12, device=DEV), m, w, c_ce=1.0)


# ---------------------------------------------------------------------------
# segment soft targets
# ---------------------------------------------------------------------------

def seg_case(V, N, vids, nids, lens, seed=0, dtype=torch.float64):
    A, S, T = len(vids), len(lens), int(sum(lens))
    rng = np.random.default_rng(seed)
    en = torch.from_numpy(np.cumsum(lens) - 1)
    st = en - torch.tensor(lens) + 1
    y = torch.from_numpy(rng.integers(0, A, T))
    y[::3] = A - 1                                # a label repeated inside every longer segment
    w = torch.from_numpy(rng.uniform(0.5, 1.5, A))
    base = _r(S, V + N, scale=2.0, seed=seed + S)
    br = base.to(dtype).clone().requires_grad_(True)
    lp = ref_logp(br, vids, nids, V, False)
    out = ref_terms(lp, w.to(dtype), 0.25 / S, 0.0, frame_label=y, st=st, en=en)
    (1.7 * out).backward()
    return dict(base=base, y=y, w=w, st=st, en=en, c_ce=0.25 / S, out=out.detach(), grad=br.grad)


def run_seg(case, m):
    bd = case["base"].float().to(DEV).requires_grad_(True)
    out = fxf.vn_class_loss(bd, m, case["w"].float().to(DEV), frame_label=case["y"].to(DEV),
                            seg_start=case["st"].to(torch.int32).to(DEV), seg_end=case["en"].to(torch.int32).to(DEV),
                            c_ce=case["c_ce"])
    (1.7 * out).backward()
    return out, bd.grad


@pytest.mark.parametrize("lens", [[1, 1, 300, 5, 1, 64], [371]], ids=["mixed", "one_segment"])
@pytest.mark.parametrize("V,N,A", [(5, 7, 12), (98, 301, 4000)])
def test_vn_loss_segment_targets(V, N, A, lens):
    """Segments of one frame, one longer than a workgroup (300 > 256 frames), and S = 1 over all rows."""
    vids, nids = _mapping(V, N, A, seed=A)
    m = fxf.VerbNounMap(vids, nids)
    case = seg_case(V, N, vids, nids, lens, seed=len(lens))
    out, grad = run_seg(case, m)
    print(f"segments {lens} A={A}: out {out.item():.8g} ref {case['out'].item():.8g}")
    np.testing.assert_allclose(out.item(), case["out"].item(), rtol=2e-5)
    _close(grad, case["grad"], what="dclogit")


def test_vn_loss_backward_is_bitwise_repeatable():
    V, N, A, R = 98, 301, 4000, 67
    vids, nids = _mapping(V, N, A, seed=1)
    m = fxf.VerbNounMap(vids, nids)
    hard = loss_case(R, V, N, vids, nids, False, True, seed=1)
    tok = loss_case(R, V, N, vids, nids, True, False, seed=2)
    seg = seg_case(V, N, vids, nids, [1, 300, 7, 40] + [2] * 63, seed=3)
    assert len(seg["st"]) == R
    runs = []
    for _ in range(2):
        o1, g1, _ = run_hard(hard, m, False)
        o2, g2, _ = run_hard(tok, m, True)
        o3, g3 = run_seg(seg, m)
        runs.append((o1, g1, o2, g2, o3, g3))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------
# prediction
# ---------------------------------------------------------------------------

def ref_eval(alp, a2f, flp, weight):
    """blocks_SepVerbNoun.py:323-342 on float64 tables; also the decision margins."""
    fprob = torch.exp(flp)
    null = alp.shape[-1] - 1
    loc = torch.where(alp.argmax(1) != null)[0]
    null_margin = float((alp[:, -1] - alp[:, :-1].max(1).values).abs().min())
    if len(loc) == 0:
        return fprob.argmax(1), fprob, null_margin
    q = torch.exp(alp[:, :-1])
    q = q / q.sum(-1, keepdim=True)
    tok = loc[a2f[:, loc].argmax(-1)]
    prob = (1 - weight) * q[tok] + weight * fprob
    return prob.argmax(1), prob, null_margin


def pair_margin(prob, vids, nids):
    """Smallest relative gap between a row's maximum and its best entry of another (verb, noun) pair."""
    pair = torch.tensor(vids) * 100000 + torch.tensor(nids)
    top = prob.argmax(1)
    other = prob.masked_fill(pair[None, :] == pair[top][:, None], -1.0)
    best = prob.max(1).values
    return float(((best - other.max(1).values) / best).min())


def eval_case(T, Q, V, N, vids, nids, seed, all_null=False):
    """Frame and token logits whose winning verb and noun are boosted by 3.0; about 40 % of the
    tokens are null; winners include actions that share their (verb, noun) pair with a lower id."""
    A = len(vids)
    rng = np.random.default_rng(seed)
    pairs = {}
    dup = [a for a in range(A) if pairs.setdefault((vids[a], nids[a]), a) != a]
    assert dup, "the mapping must hold duplicate pairs"
    fwin = rng.integers(0, A, T)
    fwin[::4] = rng.choice(dup, len(fwin[::4]))
    qwin = rng.integers(0, A, Q)
    qwin[::3] = rng.choice(dup, len(qwin[::3]))
    isnull = rng.random(Q) < 0.4
    isnull[0], isnull[-1] = False, True
    if all_null:
        isnull[:] = True
    fl = rng.standard_normal((T, V + N)) * 0.1
    fl[np.arange(T), np.asarray(vids)[fwin]] += 3.0
    fl[np.arange(T), V + np.asarray(nids)[fwin]] += 3.0
    al = rng.standard_normal((Q, V + N + 2)) * 0.1
    qv = np.where(isnull, V, np.asarray(vids)[qwin])
    qn = np.where(isnull, N, np.asarray(nids)[qwin])
    al[np.arange(Q), qv] += 3.0
    al[np.arange(Q), V + 1 + qn] += 3.0
    attn = torch.softmax(torch.from_numpy(rng.standard_normal((T, Q))).float(), -1)
    fl, al = torch.from_numpy(fl).float(), torch.from_numpy(al).float()
    return fl, al, attn, dup


EVAL_SHAPES = [(1, 3, SEG_V, SEG_N, 12), (65, 7, SEG_V, SEG_N, 12), (300, 67, 98, 301, 4000)]


def _eval_mapping(V, N, A):
    return (list(SEG_VIDS), list(SEG_NIDS)) if A == 12 else _mapping(V, N, A, seed=A)


@pytest.mark.parametrize("all_null", [False, True])
@pytest.mark.parametrize("T,Q,V,N,A", EVAL_SHAPES)
def test_vn_eval_pred(T, Q, V, N, A, all_null):
    from factmx.models.blocks_SepVerbNoun import Block
    vids, nids = _eval_mapping(V, N, A)
    m = fxf.VerbNounMap(vids, nids)
    mwt = 0.3
    fl, al, attn, dup = eval_case(T, Q, V, N, vids, nids, seed=T + Q, all_null=all_null)
    flp = ref_logp(fl.double(), vids, nids, V, False)
    alp = ref_logp(al.double(), vids, nids, V + 1, True)
    want, prob, null_margin = ref_eval(alp, attn.double(), flp, mwt)
    margin = pair_margin(prob, vids, nids)
    print(f"T={T} Q={Q} A={A} all_null={all_null}: pair margin {margin:.3f}, null margin {null_margin:.3f}")
    assert margin >= 1e-3 and null_margin >= 1e-3
    if T >= 65:
        assert np.isin(want.numpy(), dup).sum() == 0, "a duplicated pair goes to its lowest action id"
    got = fxf.vn_eval_pred(al.to(DEV), fl.to(DEV), attn.to(DEV).unsqueeze(0), m, mwt)
    assert got.dtype == torch.int64 and got.device.type == "cuda"
    np.testing.assert_array_equal(got.cpu().numpy(), want.numpy())
    # today's eager path on the materialised fp32 tables
    eager = Block._eval(fxf.verb_noun_logp(al.to(DEV), m, action=True).unsqueeze(1), attn.to(DEV).unsqueeze(0),
                        fxf.verb_noun_logp(fl.to(DEV), m).unsqueeze(1), mwt)
    assert torch.equal(got, eager)
    # segment-level attention: rows 2 t' with seg_id = the frames taken in runs of three
    seg_id = (torch.arange(T) // 3).to(torch.int32)
    S = int(seg_id.max()) + 1
    want_s, _, _ = ref_eval(alp, attn.double()[:S][seg_id.long()], flp, mwt)
    got_s = fxf.vn_eval_pred(al.to(DEV), fl.to(DEV), attn[:S].to(DEV), m, mwt, seg_id=seg_id.to(DEV))
    np.testing.assert_array_equal(got_s.cpu().numpy(), want_s.numpy())


# ---------------------------------------------------------------------------
# memory: no T x A table
# ---------------------------------------------------------------------------

def test_no_table_sized_allocation():
    from factmx.configs import get_cfg_defaults
    from factmx.models.loss import MatchCriterion
    T, V, N, A, Q = 2048, 98, 301, 4000, 32
    table = T * A * 4
    vids, nids = _mapping(V, N, A, seed=5)
    m = fxf.VerbNounMap(vids, nids)
    cfg = get_cfg_defaults()
    crit = MatchCriterion(cfg, A, [])
    label = torch.from_numpy(np.repeat(np.random.default_rng(0).integers(0, A, 64), 32)).to(DEV)
    crit.set_label(label)
    cl = _r(T, V + N, scale=2.0, seed=9).float().to(DEV).requires_grad_(True)
    al = _r(Q, V + N + 2, seed=10).float().to(DEV)
    attn = torch.softmax(_r(T, Q, seed=11).float().to(DEV), -1)
    m.tables(cl.device), m.csr(cl.device, V, N)               # the mapping's tables are made once per model
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = crit.vn_frame_terms(cl, m, ce_coef=0.25, sm_coef=5.0)
    out.backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"vn_frame_terms fwd + bwd at T={T}, A={A}: peak rise {rise / 1e6:.2f} MB (one table {table / 1e6:.1f} MB)")
    assert rise < table
    assert crit.__dict__["_onehot_class_label"] is None
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    pred = fxf.vn_eval_pred(al, cl.detach(), attn, m, 0.3)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"vn_eval_pred at T={T}, A={A}: peak rise {rise / 1e6:.2f} MB")
    assert rise < table and tuple(pred.shape) == (T,)


# ---------------------------------------------------------------------------
# MatchCriterion.vn_*_terms: the coefficient conventions against the eager CPU forms
# ---------------------------------------------------------------------------

def test_vn_terms_equal_their_cpu_forms():
    from factmx.configs import get_cfg_defaults
    from factmx.models.basic import TemporalDownsampleUpsample
    from factmx.models.loss import MatchCriterion
    V, N, A, T, Q = 5, 7, 12, 67, 9
    vids, nids = _mapping(V, N, A)
    m = fxf.VerbNounMap(vids, nids)
    cfg = get_cfg_defaults()
    cfg.Loss.nullw, cfg.Loss.bgw = 0.3, 0.5
    label = torch.from_numpy(np.repeat([3, 7, 0, 11, 3, 5], [9, 1, 20, 12, 5, 20]))
    cuts = [0, 4, 5, 30, 31, 50, T]
    st, en = torch.tensor(cuts[:-1], dtype=torch.int32), torch.tensor(cuts[1:], dtype=torch.int32) - 1
    sid = torch.repeat_interleave(torch.arange(6, dtype=torch.int32), (en - st + 1).long())
    match = (torch.tensor([4, 0, 7, 2, 8, 5]), torch.arange(6))
    fcl, scl, acl = _r(T, V + N, scale=2.0, seed=1), _r(6, V + N, scale=2.0, seed=2), _r(Q, V + N + 2, seed=3)
    res = {}
    for dev in ("cpu", DEV):
        crit = MatchCriterion(cfg, A, bg_ids=[0])
        crit.set_label(label.to(dev))
        tdu = TemporalDownsampleUpsample(sid.to(dev), st.to(dev), en.to(dev))
        cast = (lambda t: t.to(dev)) if dev == "cpu" else (lambda t: t.float().to(dev))
        res[dev] = [float(crit.vn_frame_terms(cast(fcl).unsqueeze(1), m, ce_coef=0.25, sm_coef=5.0)),
                    float(crit.vn_frame_terms(cast(fcl), m)),
                    float(crit.vn_seg_terms(cast(scl).unsqueeze(1), m, tdu, ce_coef=0.25)),
                    float(crit.vn_token_terms(match, cast(acl).unsqueeze(1), m, 0.5))]
    print("vn_*_terms cpu fp64", res["cpu"], "gpu", res[DEV])
    np.testing.assert_allclose(res[DEV], res["cpu"], rtol=2e-5)


# ---------------------------------------------------------------------------
# the model: tiny_vn with FUSED_LOSS on and off
# ---------------------------------------------------------------------------

def _tiny_vn_step(fused, monkeypatch, spy=None):
    from factmx.models import blocks_SepVerbNoun as vn
    from factmx.models.loss import MatchCriterion
    monkeypatch.setattr(vn, "FUSED_LOSS", fused)
    fx = load_fixture("tiny_vn")
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
    if spy is not None:
        real = fxf.verb_noun_logp

        def logp_spy(clogit, *a, **k):
            spy.append(int(clogit.shape[0]))
            return real(clogit, *a, **k)
        monkeypatch.setattr(fxf, "verb_noun_logp", logp_spy)
    feats, label, _ = tiny_inputs(meta)
    total, saves = net([torch.from_numpy(feats).float().to(DEV)], [torch.from_numpy(label).to(DEV)],
                       compute_loss=True)
    total.backward()
    torch.cuda.synchronize()
    if spy is not None:
        monkeypatch.setattr(fxf, "verb_noun_logp", real)
    return fx, meta, net, total, saves, captured["m"]


def test_tiny_vn_fused_vs_eager_vs_reference(monkeypatch):
    seen = []
    fx, meta, net, total, saves, match = _tiny_vn_step(True, monkeypatch, spy=seen)
    ntok = int(net.block_list[-1].action_logp.shape[0])
    assert seen and set(seen) == {ntok} and ntok != meta["T"], "only the token rows were materialised"
    _, _, net0, total0, saves0, match0 = _tiny_vn_step(False, monkeypatch)
    print(f"tiny_vn loss: fused {total.item():.8g} eager {total0.item():.8g} reference {fx['loss'][0]:.8g}")
    for tot, sv, mt in ((total, saves, match), (total0, saves0, match0)):
        np.testing.assert_allclose(tot.item(), fx["loss"][0], rtol=2e-5)
        np.testing.assert_array_equal(sv[0]["pred"], fx["pred"])
        np.testing.assert_array_equal(mt[0].numpy(), fx["match_a"])
        np.testing.assert_array_equal(mt[1].numpy(), fx["match_s"])
    np.testing.assert_allclose(total.item(), total0.item(), rtol=2e-5)
    np.testing.assert_allclose(saves[0]["loss"]["loss"], fx["loss"][0], rtol=2e-5)
    for n, prm in net.named_parameters():
        g = prm.grad
        assert g is not None, n
        rms = float(fx[f"gradsum/{n}"][1]) / np.sqrt(g.numel())
        check_grad(fx, "", n, g.cpu(), rtol=2e-3, atol=2e-3 * rms + 1e-6)
    # the side-channel tables resolve on first read to what the eager path stores
    for i, blk in enumerate(net.block_list):
        assert "_lz_frame_logp" in blk.__dict__ and not torch.is_tensor(blk.__dict__["_lz_frame_logp"])
        for k in ("frame_logp", "seg_logp", "action_logp"):
            got = getattr(blk, k)
            assert got.dim() == 3 and got.shape[1] == 1
            np.testing.assert_allclose(got[:, 0].detach().cpu().numpy(), fx[f"block{i}/{k}"], rtol=1e-4, atol=1e-4)
            np.testing.assert_allclose(got.detach().cpu().numpy(),
                                       getattr(net0.block_list[i], k).detach().cpu().numpy(), rtol=0, atol=1e-5)
        assert tuple(blk.frame_logp.shape) == (meta["T"], 1, meta["C"])
        assert getattr(blk, "frame_logp") is blk.frame_logp
