"""The verb/noun class-head kernels (csrc/verbnoun.hip) and the EPIC-Kitchens FACT built on them (GPU).

Ops are checked against a float64 torch restatement of the reference's few lines of math
(blocks_SepVerbNoun.py:189-232, 285-296); the model end to end against the ``tiny_vn`` fixture
captured from the reference itself.

Tolerances.  Kernel level: ``_close`` bounds the largest error by 2e-5 x (1 + the reference's largest
magnitude), as tests/test_gpu_kernels.py does for the other row kernels.  fp32 has u = 6e-8; a
softmax / log-softmax entry carries a few u; the longest sum here (4000 upstream gradients of
N(0, 1) into one bin, or a row's total) has partial sums up to ~sqrt(4000) = 63 and a rounding error
of about sqrt(n) u x that = 2.4e-4 at a reference magnitude of ~60-200, i.e. ~2e-6 relative -- a
tenth of the bound.  End to end: the bounds of tests/test_gpu_parity.py for the same quantities
(log-probabilities 1e-4, attention 1e-5, attention logits 1e-4, loss 2e-5 relative, gradients rtol 2e-3
+ 2e-3 x RMS + 1e-6).  The reference's own float32 run sits 3.5e-6 / 1.9e-7 / 1.6e-6 / 3.7e-8 from its
float64 run and its gradients use 1.7 % of their bound (make_golden_vn.py --spread), all under one
third of the listed bounds, which therefore stand.
"""
import numpy as np
import pytest
import torch

import paramgen as pg
from factmx import functional as fxf
from factmx import native as nx
from helpers import load_fixture, tiny_meta, cfg_from_meta, tiny_inputs, check_grad
from oracle import segments as sg

pytestmark = pytest.mark.gpu
DEV = "cuda"

FIXTURE_VIDS = [0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 0, 2]
FIXTURE_NIDS = [0, 1, 2, 3, 4, 5, 6, 0, 1, 2, 3, 6]


def _r(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


def _close(a, b, rtol=2e-5, atol=2e-5, what=""):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = (a - b).abs().max().item() if a.numel() else 0.0
    ref = b.abs().max().item() if b.numel() else 0.0
    assert err <= atol + rtol * ref, f"{what}: max err {err:.3e} (ref max {ref:.3e})"


def _mapping(V, N, A, seed=0):
    """A ids each for verbs / nouns that reach the last verb and the last noun."""
    if (V, N, A) == (5, 7, 12):
        return list(FIXTURE_VIDS), list(FIXTURE_NIDS)
    rng = np.random.default_rng(seed)
    vids, nids = rng.integers(0, V, A), rng.integers(0, N, A)
    vids[-1], nids[-1] = V - 1, N - 1
    return vids.tolist(), nids.tolist()


# ---------------------------------------------------------------------------
# process_feature(class_sep=)
# ---------------------------------------------------------------------------

def _ref_process_feature(x, n1, n2):
    f = x.shape[1] - n1 - n2
    cl = x[:, f:]
    out = torch.cat([x[:, :f], torch.softmax(cl[:, :n1], -1), torch.softmax(cl[:, n1:], -1)], -1)
    return out, cl


@pytest.mark.parametrize("with_dclogit", [False, True])
@pytest.mark.parametrize("cols,n1,n2", [(48, 5, 7), (520, 98, 301)])
@pytest.mark.parametrize("rows", [1, 3, 67])
def test_process_feature_two_groups(rows, cols, n1, n2, with_dclogit):
    wide = _r(rows, cols + 9, seed=rows + cols)                # the op reads a column slice: ld > cols
    g, gc = _r(rows, cols, seed=2), _r(rows, n1 + n2, seed=3)
    wd = wide.float().to(DEV).requires_grad_(True)
    xd = wd[:, 3:3 + cols]
    assert xd.stride(0) > cols
    out, cl = fxf.process_feature(xd, n1 + n2, class_sep=n1)
    lo = (out * g.float().to(DEV)).sum()
    if with_dclogit:
        lo = lo + (cl * gc.float().to(DEV)).sum()
    lo.backward()
    wr = wide.clone().requires_grad_(True)
    outr, clr = _ref_process_feature(wr[:, 3:3 + cols], n1, n2)
    lr = (outr * g).sum()
    if with_dclogit:
        lr = lr + (clr * gc).sum()
    lr.backward()
    _close(out, outr, what="out")
    assert torch.equal(cl.cpu(), wide.float()[:, 3 + cols - n1 - n2:3 + cols]), "clogit is a copy of the logits"
    _close(wd.grad, wr.grad, what="dx")
    f = cols - n1 - n2
    s = out.detach().double().cpu()
    np.testing.assert_allclose(s[:, f:f + n1].sum(1).numpy(), 1.0, atol=1e-5)
    np.testing.assert_allclose(s[:, f + n1:].sum(1).numpy(), 1.0, atol=1e-5)


def test_process_feature_default_path_unchanged():
    x = _r(37, 64, seed=5).float().to(DEV)
    a, ca = fxf.process_feature(x, 11)
    b, cb = fxf.process_feature(x, 11, class_sep=None)
    assert torch.equal(a, b) and torch.equal(ca, cb)
    with pytest.raises(ValueError):
        fxf.process_feature(x, 11, class_sep=11)


# ---------------------------------------------------------------------------
# verb_noun_logp
# ---------------------------------------------------------------------------

def _ref_logp(cl, vids, nids, n1, action):
    lv, ln = torch.log_softmax(cl[:, :n1], -1), torch.log_softmax(cl[:, n1:], -1)
    a = lv[:, vids] + ln[:, nids]
    if action:
        a = torch.cat([a, (lv[:, -1] + ln[:, -1]).unsqueeze(-1)], -1)
    return a


def _logp_case(R, V, N, vids, nids, action, pad=0, seed=0):
    k = 1 if action else 0
    n1, n2, A = V + k, N + k, len(vids)
    m = fxf.VerbNounMap(vids, nids)
    base = _r(R, n1 + n2 + pad, scale=2.0, seed=seed + R)
    g = _r(R, A + k, seed=seed + 7)
    bd = base.float().to(DEV).requires_grad_(True)
    cl = bd[:, pad // 2:pad // 2 + n1 + n2]
    assert (m.num_verbs, m.num_nouns) == (V, N)
    lp = fxf.verb_noun_logp(cl, m, action=action)
    (lp * g.float().to(DEV)).sum().backward()
    br = base.clone().requires_grad_(True)
    lpr = _ref_logp(br[:, pad // 2:pad // 2 + n1 + n2], vids, nids, n1, action)
    (lpr * g).sum().backward()
    _close(lp, lpr, what="logp")
    _close(bd.grad, br.grad, what="dclogit")
    return m, cl, g


@pytest.mark.parametrize("action", [False, True])
@pytest.mark.parametrize("V,N,A", [(5, 7, 1), (5, 7, 12), (98, 301, 4000)])
@pytest.mark.parametrize("R", [1, 3, 67])
def test_verb_noun_logp(R, V, N, A, action):
    vids, nids = _mapping(V, N, A, seed=A)
    _logp_case(R, V, N, vids, nids, action)


@pytest.mark.parametrize("action", [False, True])
def test_verb_noun_logp_empty_and_crowded_bins_strided(action):
    """Verb 3 owns no action, verb 2 owns 300 (> one workgroup of 256 threads); the logits are a
    column slice of a wider tensor (ld > n1 + n2)."""
    V, N, A = 6, 9, 700
    rng = np.random.default_rng(3)
    vids = np.concatenate([np.full(300, 2), rng.choice([0, 1, 4, 5], A - 300)])
    rng.shuffle(vids)
    vids[-1] = 5
    nids = rng.integers(0, N, A)
    nids[0] = N - 1
    m, cl, _ = _logp_case(5, V, N, vids.tolist(), nids.tolist(), action, pad=10)
    assert cl.stride(0) > cl.shape[1]
    voff = m.csr_host(V + int(action), N + int(action))[0]
    assert voff[4] - voff[3] == 0 and voff[3] - voff[2] == 300


def test_verb_noun_logp_transposed_input():
    """A logit tensor without unit column stride is made contiguous first."""
    vids, nids = _mapping(5, 7, 12)
    m = fxf.VerbNounMap(vids, nids)
    x = _r(12, 9, seed=4)
    lp = fxf.verb_noun_logp(x.float().to(DEV).t(), m)
    _close(lp, _ref_logp(x.t(), vids, nids, 5, False), what="logp of a transposed view")


@pytest.mark.parametrize("action", [False, True])
def test_verb_noun_logp_no_rows(action):
    k = int(action)
    vids, nids = _mapping(5, 7, 12)
    m = fxf.VerbNounMap(vids, nids)
    cl = torch.empty(0, 12 + 2 * k, device=DEV, requires_grad=True)
    lp = fxf.verb_noun_logp(cl, m, action=action)
    assert tuple(lp.shape) == (0, 12 + k)
    lp.sum().backward()
    assert tuple(cl.grad.shape) == (0, 12 + 2 * k)


def test_verb_noun_logp_backward_is_bitwise_repeatable():
    V, N, A, R = 98, 301, 4000, 67
    vids, nids = _mapping(V, N, A, seed=1)
    m = fxf.VerbNounMap(vids, nids)
    cl = _r(R, V + N + 2, scale=2.0, seed=1).float().to(DEV)
    g = _r(R, A + 1, seed=2).float().to(DEV)
    grads = []
    for _ in range(2):
        x = cl.clone().requires_grad_(True)
        (fxf.verb_noun_logp(x, m, action=True) * g).sum().backward()
        grads.append(x.grad)
    assert torch.equal(grads[0], grads[1])


def test_heads_that_do_not_fit_the_mapping_are_refused():
    m = fxf.VerbNounMap([0, 4], [6, 0])
    with pytest.raises(ValueError):
        fxf.verb_noun_logp(torch.zeros(2, 11, device=DEV), m)               # 5 + 7 logits needed
    with pytest.raises(ValueError):
        fxf.verb_noun_logp(torch.zeros(2, 12, device=DEV), m, action=True)  # 6 + 8 with the null bins
    with pytest.raises(ValueError):
        fxf.segments_from_vn_probs(torch.zeros(2, 11, device=DEV), 0, 4, 7, m)
    lib = nx.load()
    st = lib.fx_vn_logp_fwd(None, 4096, 1, 2000, 2000, None, None, 4, 0, None, 4, None, None)
    assert st != 0 and b"2048" in lib.fx_last_error()


# ---------------------------------------------------------------------------
# segments_from_vn_probs
# ---------------------------------------------------------------------------

SEG_V, SEG_N = 5, 7
# actions 3 and 9 are the same (verb, noun) pair: their products are equal on every frame
SEG_VIDS = [0, 1, 2, 3, 4, 0, 1, 2, 3, 3, 0, 2]
SEG_NIDS = [0, 1, 2, 3, 4, 5, 6, 0, 1, 3, 3, 6]


def _vn_probs(T, col0, seed):
    """fp32 (T, col0 + V + N) rows: col0 feature columns, then verb and noun probabilities whose
    winning action stays for a few frames; every fifth frame is won by the duplicated pair (3, 3)."""
    rng = np.random.default_rng(seed)
    runs = np.repeat(rng.integers(0, len(SEG_VIDS), T), rng.integers(1, 6, T))[:T]
    runs[::5] = 9
    lv = rng.standard_normal((T, SEG_V)).astype(np.float32) * 0.1
    ln = rng.standard_normal((T, SEG_N)).astype(np.float32) * 0.1
    lv[np.arange(T), np.asarray(SEG_VIDS)[runs]] += 3.0
    ln[np.arange(T), np.asarray(SEG_NIDS)[runs]] += 3.0
    pv = torch.softmax(torch.from_numpy(lv), -1)
    pn = torch.softmax(torch.from_numpy(ln), -1)
    feat = torch.from_numpy(rng.standard_normal((T, col0)).astype(np.float32))
    return torch.cat([feat, pv, pn], -1).contiguous()


def _ref_segments(x, col0):
    """torch fp32 product + first-maximum argmax, then the run-length encoding."""
    pv, pn = x[:, col0:col0 + SEG_V], x[:, col0 + SEG_V:col0 + SEG_V + SEG_N]
    prod = pv[:, SEG_VIDS] * pn[:, SEG_NIDS]
    assert prod.dtype == torch.float32
    pred = prod.argmax(-1).numpy()
    _, st, en = sg.run_length_segments(pred)
    return pred, np.asarray(st), np.asarray(en), sg.segment_ids_from_bounds(st, en, len(pred))


@pytest.mark.parametrize("T", [1, 2, 65, 300])
def test_segments_from_vn_probs(T):
    col0 = 36
    x = _vn_probs(T, col0, seed=T)
    pred, st, en, sid = _ref_segments(x, col0)
    if T >= 65:
        tie = (x[:, col0 + 3] * x[:, col0 + SEG_V + 3]) >= (x[:, col0:col0 + SEG_V][:, SEG_VIDS]
                                                             * x[:, col0 + SEG_V:][:, SEG_NIDS]).max(-1).values
        assert tie.any() and (pred[tie.numpy()] == 3).all(), "tied frames must exist and go to the first index"
        assert not (pred == 9).any()
    m = fxf.VerbNounMap(SEG_VIDS, SEG_NIDS)
    S, seg_id, s32, e32 = fxf.segments_from_vn_probs(x.to(DEV), col0, SEG_V, SEG_N, m)
    assert S == len(st)
    np.testing.assert_array_equal(s32.cpu().numpy(), st)
    np.testing.assert_array_equal(e32.cpu().numpy(), en)
    np.testing.assert_array_equal(seg_id.cpu().numpy(), sid)
    from factmx.models.basic import TemporalDownsampleUpsample
    tdu = TemporalDownsampleUpsample.from_vn_probs(x.to(DEV), col0, SEG_V, SEG_N, m)
    assert tdu.num_seg == S and torch.equal(tdu.start32, s32)


def test_segments_from_vn_probs_two_ragged_videos():
    """The batched C entry: two videos of 65 and 300 rows, video-local tables, pred included."""
    lib = nx.load()
    col0, Ts = 4, [65, 300]
    xs = [_vn_probs(T, col0, seed=10 + T) for T in Ts]
    x = torch.cat(xs, 0).to(DEV)
    n = sum(Ts)
    m = fxf.VerbNounMap(SEG_VIDS, SEG_NIDS)
    vids, nids = m.tables(x.device)
    buf = torch.full((4 * n + 2,), -1, device=DEV, dtype=torch.int32)
    pred, seg_id, st, en, ns = buf[:n], buf[n:2 * n], buf[2 * n:3 * n], buf[3 * n:4 * n], buf[4 * n:]
    nx.check(lib.fx_segments_from_vn_probs(nx.ptr(x), nx.ld(x), col0, SEG_V, SEG_N, nx.ptr(vids), nx.ptr(nids),
                                           len(SEG_VIDS), 0, 2, nx.int_array([0, Ts[0], n]), nx.ptr(pred),
                                           nx.ptr(seg_id), nx.ptr(st), nx.ptr(en), nx.ptr(ns), nx.stream()),
             "fx_segments_from_vn_probs")
    counts = ns.cpu().tolist()
    off = 0
    for v, T in enumerate(Ts):
        p_ref, s_ref, e_ref, id_ref = _ref_segments(xs[v], col0)
        assert counts[v] == len(s_ref)
        np.testing.assert_array_equal(pred[off:off + T].cpu().numpy(), p_ref)
        np.testing.assert_array_equal(seg_id[off:off + T].cpu().numpy(), id_ref)
        np.testing.assert_array_equal(st[off:off + counts[v]].cpu().numpy(), s_ref)
        np.testing.assert_array_equal(en[off:off + counts[v]].cpu().numpy(), e_ref)
        off += T


# ---------------------------------------------------------------------------
# end to end: tiny_vn
# ---------------------------------------------------------------------------

def test_transcript_conditioned_model_runs():
    """FACT.trans: tokens are verb / noun embeddings of the transcript (blocks_SepVerbNoun.py:78-86) and
    the prediction picks transcript entries; every parameter gets a finite gradient."""
    from factmx.models import blocks_SepVerbNoun as vn
    from factmx.models.loss import MatchCriterion
    fx = load_fixture("tiny_vn")
    meta = tiny_meta(fx)
    cfg = cfg_from_meta(meta)
    cfg.FACT.trans = True
    vn.set_verb_noun_ids(fx["vids"].tolist(), fx["nids"].tolist())
    net = vn.FACT(cfg, meta["D"], meta["V"], meta["N"])
    with torch.no_grad():
        for n, p in net.named_parameters():
            p.copy_(torch.from_numpy(pg.param_value(n, p.shape, 3)))
    net.mcriterion = MatchCriterion(cfg, meta["C"], [])
    net = net.to(DEV).train()
    feats, label, _ = tiny_inputs(meta)
    total, saves = net([torch.from_numpy(feats).float().to(DEV)], [torch.from_numpy(label).to(DEV)],
                       compute_loss=True)
    total.backward()
    assert np.isfinite(total.item())
    assert set(saves[0]["pred"].tolist()) <= set(label.tolist())
    for n, p in net.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
    assert net.verb_embed.weight.grad.abs().sum() > 0 and net.noun_embed.weight.grad.abs().sum() > 0


def test_tiny_vn_end_to_end_vs_reference():
    from factmx.models import blocks_SepVerbNoun as vn
    from factmx.models.loss import MatchCriterion
    fx = load_fixture("tiny_vn")
    meta = tiny_meta(fx)
    cfg = cfg_from_meta(meta)
    vn.set_verb_noun_ids(fx["vids"].tolist(), fx["nids"].tolist())
    net = vn.FACT(cfg, meta["D"], meta["V"], meta["N"])
    assert {n: list(p.shape) for n, p in net.named_parameters()} == meta["param_shapes"]
    with torch.no_grad():
        for n, p in net.named_parameters():
            p.copy_(torch.from_numpy(pg.param_value(n, p.shape, meta["seed"])))
    net.mcriterion = MatchCriterion(cfg, meta["C"], [])
    net = net.to(DEV).train()
    captured = {}
    orig = net.mcriterion.match

    def spy(*a, **k):
        captured["m"] = orig(*a, **k)
        return captured["m"]
    net.mcriterion.match = spy
    feats, label, _ = tiny_inputs(meta)
    total, saves = net([torch.from_numpy(feats).float().to(DEV)], [torch.from_numpy(label).to(DEV)],
                       compute_loss=True)
    total.backward()
    torch.cuda.synchronize()

    for i, blk in enumerate(net.block_list):
        p = f"block{i}/"
        np.testing.assert_array_equal(blk.tdu.start32.cpu().numpy(), fx[p + "seg_start"], err_msg=p)
        np.testing.assert_array_equal(blk.tdu.end32.cpu().numpy(), fx[p + "seg_end"], err_msg=p)
        for k in ("frame_logp", "seg_logp", "action_logp"):
            got = getattr(blk, k)
            assert got.dim() == 3 and got.shape[1] == 1
            np.testing.assert_allclose(got[:, 0].detach().cpu().numpy(), fx[p + k], rtol=1e-4, atol=1e-4,
                                       err_msg=p + k)
        if i == 0:
            assert blk.a2f_attn is None and blk.f2a_attn is None
            continue
        np.testing.assert_allclose(blk.a2f_attn[0].detach().cpu().numpy(), fx[p + "a2f_attn"], atol=1e-5)
        for k in ("f2a_attn_logit", "a2f_attn_logit"):
            np.testing.assert_allclose(getattr(blk, k)[0].detach().cpu().numpy(), fx[p + k], rtol=1e-4, atol=1e-4,
                                       err_msg=p + k)
    np.testing.assert_array_equal(saves[0]["pred"], fx["pred"])
    np.testing.assert_array_equal(captured["m"][0].numpy(), fx["match_a"])
    np.testing.assert_array_equal(captured["m"][1].numpy(), fx["match_s"])
    np.testing.assert_allclose(total.item(), fx["loss"][0], rtol=2e-5)
    np.testing.assert_allclose(saves[0]["loss"]["loss"], fx["loss"][0], rtol=2e-5)
    for n, prm in net.named_parameters():
        g = prm.grad
        assert g is not None, n
        rms = float(fx[f"gradsum/{n}"][1]) / np.sqrt(g.numel())
        check_grad(fx, "", n, g.cpu(), rtol=2e-3, atol=2e-3 * rms + 1e-6)
