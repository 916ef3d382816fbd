"""The lockstep step of the verb/noun FACT (GPU): fx_vn_match_cost_batch / fx_vn_eval_pred_batch
(csrc/vnloss.hip), functional.segments_from_vn_probs_batched and blocks_SepVerbNoun.LOCKSTEP.

Kernel level: every batched entry against its single-video twin (bitwise / equal) and, for the cost, against
the float64 restatement of tests/vn_cases.py within 2e-5 x (1 + max|ref|) (DESIGN.md section 7n's bound).
Model level: the ``tiny_vn_batch`` fixture (three ragged videos through the reference in float64) with the
bounds of section 7l: losses rtol 2e-5, gradients rtol 2e-3 + 2e-3 RMS + 1e-6; the same step on the
per-video path within the same bounds.
"""
import numpy as np
import pytest
import torch

import paramgen as pg
import vn_cases as vc
from factmx import functional as fxf
from factmx import native as nx
from helpers import load_fixture, tiny_meta, cfg_from_meta, tiny_inputs, check_grad
from test_gpu_verbnoun import _vn_probs, SEG_V, SEG_N, SEG_VIDS, SEG_NIDS

pytestmark = pytest.mark.gpu
DEV = "cuda"
PC, A2FC, MWT = 0.2, 1.0, 0.1

SMALL = (5, 7, 12)
BIG = (98, 301, 4000)
# (T, G, S): a one-frame video, S = T with G < Gmax, and several blocks' worth of frames with S < T
RAGGED = [(1, 1, 1), (33, 2, 33), (211, 5, 40)]


def i32(a):
    return torch.from_numpy(np.asarray(a, dtype=np.int32)).to(DEV)


def make_video(T, Q, G, S, heads, seed, null_tokens=False):
    """One video of a batch: token heads, ground truth, S TDU intervals, the (S, Q) segment attention, its
    (T, Q) frame-level gather and frame heads; all videos of one ``heads`` share the mapping."""
    V, N, A = heads
    case = vc.match_case(T, Q, G, V, N, A, seed=seed)
    rng = np.random.default_rng(seed + 1)
    st, en = vc.intervals(vc.cuts(T, S, rng))
    seg, frame = vc.seg_attention(case, st, en)
    if null_tokens:                       # every token's first maximum is the null column
        case["acl"][:, V] += 30.0
        case["acl"][:, V + 1 + N] += 30.0
    fcl = torch.from_numpy(rng.standard_normal((T, V + N)).astype(np.float32) * 2.0)
    seg_id = np.repeat(np.arange(S), en - st + 1).astype(np.int32)
    return dict(case=case, st=st, en=en, seg=seg, frame=frame, fcl=fcl, seg_id=seg_id, T=T, Q=Q, G=G, S=S)


def batch(shapes, Q, heads, null_video=None):
    return [make_video(T, Q, G, S, heads, seed=11 * T + G + 3 * v, null_tokens=(v == null_video))
            for v, (T, G, S) in enumerate(shapes)]


def vnmap_of(videos):
    c = videos[0]["case"]
    return fxf.VerbNounMap(c["vids"], c["nids"])


def cost_args(v, level):
    c = v["case"]
    d = dict(action_clogit=c["acl"].to(DEV), gs=i32(c["gs"]), ge=i32(c["ge"]), gl=i32(c["gl"]), T=v["T"])
    if level == "seg":
        d.update(attn=v["seg"].to(DEV), seg_start=i32(v["st"]), seg_end=i32(v["en"]))
    else:
        d.update(attn=v["frame"].to(DEV))
    return d


def check_cost_batch(videos, level):
    m = vnmap_of(videos)
    args = [cost_args(v, level) for v in videos]
    got = fxf.vn_match_cost_batch(args, m, PC, A2FC)
    again = fxf.vn_match_cost_batch(args, m, PC, A2FC)
    Gmax = max(v["G"] for v in videos)
    assert tuple(got.shape) == (len(videos), videos[0]["Q"], Gmax) and got.dtype == torch.float32
    assert torch.equal(got, again), "two runs differ"
    for i, (v, a) in enumerate(zip(videos, args)):
        G = v["G"]
        one = fxf.vn_match_cost(a["action_clogit"], a["attn"], m, a["gs"], a["ge"], a["gl"], a["T"], PC, A2FC,
                                seg_start=a.get("seg_start"), seg_end=a.get("seg_end"))
        assert torch.equal(got[i, :, :G], one), f"video {i}: not bitwise the single-video cost"
        assert not bool(got[i, :, G:].ne(0).any()), f"video {i}: padding not zero"
        ref = vc.ref_cost(v["case"], v["frame"], PC, A2FC, device=DEV)
        err = float((got[i, :, :G].double() - ref).abs().max())
        lim = vc.BOUND * (1.0 + float(ref.abs().max()))
        print(f"{level} video {i} T={v['T']} G={G} S={v['S']}: max err {err:.3e} (bound {lim:.3e})")
        assert err <= lim


# ---------------------------------------------------------------------------
# vn_match_cost_batch
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("level", ["seg", "frame"])
@pytest.mark.parametrize("shapes", [RAGGED[2:], RAGGED], ids=["nvid1", "nvid3"])
def test_match_cost_batch(shapes, level):
    check_cost_batch(batch(shapes, 8, SMALL), level)


def test_match_cost_batch_wide_heads():
    check_cost_batch(batch(RAGGED, 8, BIG), "seg")


def test_match_cost_batch_70_tokens_70_segments():
    check_cost_batch(batch([(300, 70, 40), (97, 3, 21)], 70, SMALL), "seg")


def test_match_cost_batch_refuses_another_token_count_before_any_launch():
    videos = batch(RAGGED, 8, SMALL)
    m = vnmap_of(videos)
    args = [cost_args(v, "seg") for v in videos]
    args[1]["attn"] = args[1]["attn"][:, :5].contiguous()
    with pytest.raises(ValueError):
        fxf.vn_match_cost_batch(args, m, PC, A2FC)
    args = [cost_args(v, "seg") for v in videos]
    args[2]["action_clogit"] = args[2]["action_clogit"][:5]
    with pytest.raises(ValueError):
        fxf.vn_match_cost_batch(args, m, PC, A2FC)


# ---------------------------------------------------------------------------
# vn_eval_pred_batch
# ---------------------------------------------------------------------------

def pred_args(v, level):
    d = dict(action_clogit=v["case"]["acl"].to(DEV), frame_clogit=v["fcl"].to(DEV))
    if level == "seg":
        d.update(attn=v["seg"].to(DEV), seg_id=i32(v["seg_id"]))
    else:
        d.update(attn=v["frame"].to(DEV))
    return d


@pytest.mark.parametrize("level", ["seg", "frame"])
@pytest.mark.parametrize("name", ["nvid1", "nvid3", "null_video", "wide", "q70"])
def test_eval_pred_batch(name, level):
    videos = {"nvid1": lambda: batch(RAGGED[2:], 8, SMALL), "nvid3": lambda: batch(RAGGED, 8, SMALL),
              "null_video": lambda: batch(RAGGED, 8, SMALL, null_video=1),
              "wide": lambda: batch(RAGGED, 8, BIG),
              "q70": lambda: batch([(300, 70, 40), (97, 3, 21)], 70, SMALL)}[name]()
    m = vnmap_of(videos)
    args = [pred_args(v, level) for v in videos]
    got = fxf.vn_eval_pred_batch(args, m, MWT)
    assert got.dtype == torch.int64 and got.shape == (sum(v["T"] for v in videos),)
    assert torch.equal(got, fxf.vn_eval_pred_batch(args, m, MWT))
    off = 0
    for i, (v, a) in enumerate(zip(videos, args)):
        one = fxf.vn_eval_pred(a["action_clogit"], a["frame_clogit"], a["attn"], m, MWT, seg_id=a.get("seg_id"))
        assert torch.equal(got[off:off + v["T"]], one), f"video {i}"
        if name == "null_video" and i == 1:      # no non-null token: the frame heads decide alone
            lp = vc.ref_logp(v["fcl"].double(), v["case"]["vids"], v["case"]["nids"], SMALL[0], False)
            top = torch.topk(lp, 2, dim=-1).values
            clear = ((top[:, 0] - top[:, 1]) > 1e-4).numpy()
            np.testing.assert_array_equal(one.cpu().numpy()[clear], lp.argmax(-1).numpy()[clear])
        off += v["T"]


def test_eval_pred_batch_refuses_bad_videos():
    videos = batch(RAGGED, 8, SMALL)
    m = vnmap_of(videos)
    args = [pred_args(v, "seg") for v in videos]
    args[2]["seg_id"] = args[2]["seg_id"][:-1]
    with pytest.raises(ValueError):
        fxf.vn_eval_pred_batch(args, m, MWT)


# ---------------------------------------------------------------------------
# segments_from_vn_probs_batched
# ---------------------------------------------------------------------------

def test_segments_from_vn_probs_batched():
    col0, Ts = 36, [65, 1, 300]
    xs = [_vn_probs(T, col0, seed=20 + T) for T in Ts]
    m = fxf.VerbNounMap(SEG_VIDS, SEG_NIDS)
    f_off = [0, 65, 66, 366]
    ran = []
    S, local, (gid, gst, gen) = fxf.segments_from_vn_probs_batched(torch.cat(xs, 0).to(DEV), col0, SEG_V, SEG_N, m,
                                                                   f_off, while_waiting=lambda: ran.append(1))
    assert ran == [1]
    s_off = 0
    for v, T in enumerate(Ts):
        S1, sid, st, en = fxf.segments_from_vn_probs(xs[v].to(DEV), col0, SEG_V, SEG_N, m)
        assert S[v] == S1
        assert torch.equal(local[v][0], sid) and torch.equal(local[v][1], st) and torch.equal(local[v][2], en)
        assert torch.equal(gid[f_off[v]:f_off[v + 1]], sid + s_off)
        assert torch.equal(gst[s_off:s_off + S1], st + f_off[v]) and torch.equal(gen[s_off:s_off + S1], en + f_off[v])
        s_off += S1
    assert gst.shape[0] == s_off
    with pytest.raises(ValueError):
        fxf.segments_from_vn_probs_batched(torch.cat(xs, 0).to(DEV), col0, SEG_V, SEG_N, m, [0, 65, 300])


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------

def _build(fixture):
    from factmx.models import blocks_SepVerbNoun as vn
    from factmx.models.loss import MatchCriterion
    fx = load_fixture(fixture)
    meta = tiny_meta(fx)
    cfg = cfg_from_meta(meta)
    vn.set_verb_noun_ids(fx["vids"].tolist(), fx["nids"].tolist())
    net = vn.FACT(cfg, meta["D"], meta["V"], meta["N"])
    with torch.no_grad():
        for n, p in net.named_parameters():
            p.copy_(torch.from_numpy(pg.param_value(n, p.shape, meta["seed"])))
    net.mcriterion = MatchCriterion(cfg, meta["C"], [])
    return fx, meta, net.to(DEV).train()


def _batch_inputs(meta):
    vids = [pg.segmented_video(T, meta["D"], meta["seen"], nseg, seed=seed, noise=meta["noise"])
            for T, nseg, seed in meta["videos"]]
    return ([torch.from_numpy(f).float().to(DEV) for f, _ in vids], [torch.from_numpy(l_).to(DEV) for _, l_ in vids])


def _step(mp, lockstep, fixture="tiny_vn_batch", spy=False, compute_loss=True, maxk=None):
    """One step of the fixture's batch; ``spy``: count the batched entries and the table launches, poison the
    per-video entries and the per-term losses."""
    from factmx.models import blocks_SepVerbNoun as vn
    from factmx.models import vloss, vn_vloss
    from factmx.models.loss import MatchCriterion
    mp.setattr(vn, "FUSED_LOSS", True)
    mp.setattr(vn_vloss, "FUSED_TABLE", True)
    mp.setattr(vn, "LOCKSTEP", lockstep)
    if maxk is not None:
        mp.setattr(nx, "LOSS_MAXK", maxk)
    fx, meta, net = _build(fixture)
    calls = {"cost": 0, "pred": 0, "table": 0}
    matches = []
    if spy:
        def counted(key, fn):
            def f(*a, **k):
                calls[key] += 1
                return fn(*a, **k)
            return f

        def boom(*a, **k):
            raise AssertionError("a per-video entry ran on the lockstep path")
        mp.setattr(fxf, "vn_match_cost_batch", counted("cost", fxf.vn_match_cost_batch))
        mp.setattr(fxf, "vn_eval_pred_batch", counted("pred", fxf.vn_eval_pred_batch))
        mp.setattr(vloss._LossFn, "apply", staticmethod(counted("table", vloss._LossFn.apply)))
        for name in ("vn_match_cost", "vn_eval_pred", "vn_class_loss"):
            mp.setattr(fxf, name, boom)
        mp.setattr(MatchCriterion, "cross_attn_loss_tdu", boom)
    else:
        orig = net.mcriterion.match

        def match_spy(*a, **k):
            matches.append(orig(*a, **k))
            return matches[-1]
        net.mcriterion.match = match_spy
    if "videos" in meta:
        seqs, labels = _batch_inputs(meta)
    else:
        feats, label, _ = tiny_inputs(meta)
        seqs, labels = [torch.from_numpy(feats).float().to(DEV)], [torch.from_numpy(label).to(DEV)]
    if not compute_loss:
        with torch.no_grad():
            saves = net(seqs, labels, compute_loss=False)
        torch.cuda.synchronize()
        return dict(fx=fx, meta=meta, net=net, saves=saves)
    total, saves = net(seqs, labels, compute_loss=True)
    total.backward()
    torch.cuda.synchronize()
    if lockstep and maxk is None:
        matches = [tuple(torch.as_tensor(x) for x in m) for m in net._matches]
    return dict(fx=fx, meta=meta, net=net, total=total, saves=saves, matches=matches, calls=calls)


@pytest.fixture(scope="module")
def steps():
    """The fixture's step on the lockstep path (spied) and on the per-video path, run once."""
    out = {}
    for key, lock in (("lock", True), ("video", False)):
        with pytest.MonkeyPatch.context() as mp:
            out[key] = _step(mp, lock, spy=lock)
    return out


def _check_grads(fx, net):
    for n, prm in net.named_parameters():
        assert prm.grad is not None, n
        rms = float(fx[f"gradsum/{n}"][1]) / np.sqrt(prm.grad.numel())
        check_grad(fx, "", n, prm.grad.cpu(), rtol=2e-3, atol=2e-3 * rms + 1e-6)


@pytest.mark.parametrize("path", ["lock", "video"])
def test_tiny_vn_batch_against_the_reference(steps, path):
    """``video``: the same step with LOCKSTEP = False, the parent's path, within the same bounds."""
    r = steps[path]
    fx, net = r["fx"], r["net"]
    nvid = int(fx["nvid"])
    print(f"{path}: batch loss {r['total'].item():.8g} reference {fx['loss'][0]:.8g}; video losses",
          [s["loss"]["loss"] for s in r["saves"]], "reference", [float(fx[f'video{v}/loss'][0]) for v in range(nvid)])
    np.testing.assert_allclose(r["total"].item(), fx["loss"][0], rtol=2e-5)
    assert len(r["saves"]) == len(r["matches"]) == nvid == 3
    for v in range(nvid):
        p = f"video{v}/"
        np.testing.assert_allclose(r["saves"][v]["loss"]["loss"], fx[p + "loss"][0], rtol=2e-5)
        np.testing.assert_array_equal(r["saves"][v]["pred"], fx[p + "pred"])
        np.testing.assert_array_equal(r["matches"][v][0].numpy(), fx[p + "match_a"])
        np.testing.assert_array_equal(r["matches"][v][1].numpy(), fx[p + "match_s"])
    _check_grads(fx, net)
    nb = len(net.block_list)
    assert len(net.loss_list) == nb
    np.testing.assert_allclose(sum(x.item() for x in net.loss_list) / nb, fx[f"video{nvid - 1}/loss"][0], rtol=2e-5)


def test_lockstep_segments_side_channels_and_launch_counts(steps):
    r = steps["lock"]
    fx, net, meta = r["fx"], r["net"], r["meta"]
    assert r["calls"] == {"cost": 1, "pred": 1, "table": 1}
    Ts = [v[0] for v in meta["videos"]]
    for v in range(3):
        for k, blk in enumerate(net.block_list):
            _, st, en = blk._bt["local"][v]
            np.testing.assert_array_equal(st.cpu().numpy(), fx[f"video{v}/block{k}/seg_start"])
            np.testing.assert_array_equal(en.cpu().numpy(), fx[f"video{v}/block{k}/seg_end"])
    assert net.video_segments == [[len(fx[f"video{v}/block{k}/seg_start"]) for k in range(3)] for v in range(3)]
    # the side channels hold the last video's values, as on the per-video path
    last, ref = net.block_list[-1], steps["video"]["net"].block_list[-1]
    T, S, Q = Ts[-1], net.video_segments[-1][-1], meta["FACT"]["ntoken"]
    assert last.tdu.num_seg == S and torch.equal(last.tdu.start32, ref.tdu.start32)
    assert tuple(last._clogits[0].shape) == (T, 1, 12) and tuple(last._clogits[1].shape) == (S, 1, 12)
    assert tuple(last._clogits[2].shape) == (Q, 1, 14) and tuple(last.action_logp.shape) == (Q, 1, 13)
    assert tuple(last.a2f_seg_attn.shape) == (1, S, Q) and tuple(last.f2a_seg_attn.shape) == (1, S, Q)
    assert tuple(last.a2f_attn_logit.shape) == (1, S, Q) and tuple(last.f2a_attn_logit.shape) == (1, Q, S)
    assert not torch.is_tensor(last.__dict__["_lz_a2f_attn"])          # lazy until read
    assert tuple(last.a2f_attn.shape) == (1, T, Q) and tuple(last.f2a_attn.shape) == (1, Q, T)
    assert tuple(last.frame_logp.shape) == (T, 1, 12) and tuple(last.seg_logp.shape) == (S, 1, 12)
    # section 7l's bounds of each quantity against float64 (attention 1e-5, logits and log-probabilities 1e-4)
    for name, rtol, atol in (("a2f_seg_attn", 0.0, 1e-5), ("f2a_seg_attn", 0.0, 1e-5), ("a2f_attn", 0.0, 1e-5),
                             ("a2f_attn_logit", 1e-4, 1e-4), ("f2a_attn_logit", 1e-4, 1e-4),
                             ("action_logp", 1e-4, 1e-4), ("frame_logp", 1e-4, 1e-4)):
        np.testing.assert_allclose(getattr(last, name).detach().cpu().numpy(),
                                   getattr(ref, name).detach().cpu().numpy(), rtol=rtol, atol=atol, err_msg=name)
    first = net.block_list[0]
    assert first.a2f_seg_attn is None and first.a2f_attn is None and first.tdu.num_seg == net.video_segments[-1][0]


def test_lockstep_agrees_with_the_per_video_path(steps):
    a, b = steps["lock"], steps["video"]
    np.testing.assert_allclose(a["total"].item(), b["total"].item(), rtol=2e-5)
    for sa, sb, ma, mb in zip(a["saves"], b["saves"], a["matches"], b["matches"]):
        np.testing.assert_allclose(sa["loss"]["loss"], sb["loss"]["loss"], rtol=2e-5)
        np.testing.assert_array_equal(sa["pred"], sb["pred"])
        assert torch.equal(ma[0], mb[0]) and torch.equal(ma[1], mb[1])
    for (n, p), (_, p0) in zip(a["net"].named_parameters(), b["net"].named_parameters()):
        rms = float(a["fx"][f"gradsum/{n}"][1]) / np.sqrt(p.grad.numel())
        np.testing.assert_allclose(p.grad.cpu().numpy(), p0.grad.cpu().numpy(), rtol=2e-3, atol=2e-3 * rms + 1e-6,
                                   err_msg=n)


def test_one_video_in_lockstep_reproduces_tiny_vn(monkeypatch):
    r = _step(monkeypatch, True, fixture="tiny_vn", spy=True)
    fx = r["fx"]
    assert r["calls"] == {"cost": 1, "pred": 1, "table": 1}
    np.testing.assert_allclose(r["total"].item(), fx["loss"][0], rtol=2e-5)
    np.testing.assert_array_equal(r["saves"][0]["pred"], fx["pred"])
    np.testing.assert_array_equal(r["matches"][0][0].numpy(), fx["match_a"])
    np.testing.assert_array_equal(r["matches"][0][1].numpy(), fx["match_s"])
    for k, blk in enumerate(r["net"].block_list):
        np.testing.assert_array_equal(blk.tdu.start32.cpu().numpy(), fx[f"block{k}/seg_start"])
    _check_grads(fx, r["net"])


def test_lockstep_predictions_without_the_loss(steps, monkeypatch):
    r = _step(monkeypatch, True, spy=True, compute_loss=False)
    assert all(set(s) == {"pred"} for s in r["saves"])
    for s, s0 in zip(r["saves"], steps["lock"]["saves"]):
        np.testing.assert_array_equal(s["pred"], s0["pred"])


def test_batch_past_the_table_limit_takes_the_per_video_losses(steps, monkeypatch):
    """Every video's match pairs more than FX_LOSS_MAXK (here 2) columns: the losses and predictions run per
    video on the lockstep outputs."""
    r = _step(monkeypatch, True, maxk=2)
    ref = steps["video"]
    assert len(r["matches"]) == 3 and all(len(m[0]) > 2 for m in r["matches"])
    np.testing.assert_allclose(r["total"].item(), ref["total"].item(), rtol=2e-5)
    for s, s0 in zip(r["saves"], ref["saves"]):
        np.testing.assert_allclose(s["loss"]["loss"], s0["loss"]["loss"], rtol=2e-5)
        np.testing.assert_array_equal(s["pred"], s0["pred"])
    assert r["net"].video_segments == steps["lock"]["net"].video_segments
    _check_grads(r["fx"], r["net"])
