"""Capture the transcript-conditioned fixtures (``FACT.trans``) from the reference's vanilla FACT
(fact_clip/models/blocks.py; build container only, like make_golden.py / make_golden_vn.py).

Run:  python tests/golden/make_golden_trans.py            # writes tiny_trans*.<i>.npz
      python tests/golden/make_golden_trans.py --spread   # the reference in float32 vs its float64 run
      python tests/golden/make_golden_trans.py --search   # the seed search behind videos B and C

Three fixtures, one tiny model family (D=40, C=12, widths as tiny_vn; nullw = 1.0: with as many tokens as
ground-truth segments tiny_vn's formula divides by zero):

  tiny_trans        block iuU, Bi.a = sca, Loss.match = seq; video A, transcript [2, 5, 9, 2, 5] (repeated
                    classes: the embedding gradient sums two rows, the prediction gathers duplicate columns)
  tiny_trans_batch  the same model; videos A, B (5 transcript entries each) and C (4): per-video losses,
                    predictions, segment bounds and the gradients of the batch-mean loss for [A, B] and [A, B, C]
  tiny_trans_gru    block iU, Bi.a = gru_om, Loss.match = o2o; video A, the matching recorded

Weights and inputs come from ``paramgen``; the fixtures hold float64 outputs and gradients.

Conditions (asserted; A's seed is the issue's, the seeds of B and C below were found by ``--search``, which
tries seeds in order until the conditions hold):
  * segmentation: the class probabilities' relative top-2 margin >= 1e-3 on every frame at every TDU
    segmentation, so that an fp32 argmax cannot move a segment boundary;
  * prediction: the blended transcript probability's relative top-2 margin on every frame >= 100 x the
    largest relative float32-vs-float64 difference of that probability (the double softmax is nearly flat,
    so the margins are small in absolute terms: the criterion is relative to the float32 error).

``--spread`` prints how far the reference's own float32 run sits from its float64 run for every compared
quantity (DESIGN.md section 7r derives the test tolerances from it).
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, os.path.join(ROOT, "fact-clip_amd"))
sys.path.insert(0, os.path.join(HERE, "_yacs_shim"))
sys.path.insert(0, REF)
sys.path.insert(0, HERE)

import torch  # noqa: E402

import paramgen as pg  # noqa: E402
from fixture_io import save_fixture  # noqa: E402
from fact_clip.configs.default import get_cfg_defaults  # noqa: E402
from fact_clip.models import blocks as rblocks  # noqa: E402
from fact_clip.models import loss as rloss  # noqa: E402

MIN_SEG_MARGIN = 1e-3
PRED_MARGIN_FACTOR = 100.0
PARAM_SEED = 1

_BI = dict(hid_dim=48, dropout=0.0, a_nhead=4, a_ffdim=48, a_layers=2, a_dim=32, f="m", f_layers=3, f_ln=False,
           f_dim=24, f_ngp=1)
_LOSS = dict(pc=0.2, a2fc=1.0, bgw=1.0, sw=5.0, nullw=1.0)

MODELS = {
    "sca": dict(model="FACT", D=40, C=12, seed=PARAM_SEED, holdout=[],
                FACT=dict(ntoken=0, block="iuU", fpos=True, cmr=0.0, mwt=0.1, trans=True),
                Bi=dict(_BI, a="sca"), Bu=dict(f_layers=3, a_nhead=4, a="sa"),
                BU=dict(f_layers=3, a_nhead=4, s_layers=1, a="sa"), Loss=dict(_LOSS, match="seq")),
    "gru": dict(model="FACT", D=40, C=12, seed=PARAM_SEED, holdout=[],
                FACT=dict(ntoken=0, block="iU", fpos=True, cmr=0.0, mwt=0.1, trans=True),
                Bi=dict(_BI, a="gru_om"), Bu=dict(f_layers=3, a_nhead=4, a="sa"),
                BU=dict(f_layers=3, a_nhead=4, s_layers=1, a="sa"), Loss=dict(_LOSS, match="o2o")),
}

VIDEO_A = dict(T=150, classes=[2, 5, 9], nseg=5, seed=1, noise=0.3)
# B: 5 transcript entries like A, so [A, B] is one pass; C: 4.  Their seeds are what ``--search`` finds from
# the starts SEARCH_FROM (B's seed 3 holds the conditions only barely: segmentation margin 1.05e-3).
VIDEO_B = dict(T=97, classes=[2, 5, 9], nseg=5, seed=4, noise=0.3)
VIDEO_C = dict(T=120, classes=list(range(12)), nseg=4, seed=2, noise=0.3)
SEARCH_FROM = dict(B=3, C=2)

SIDE_KEYS = ("frame_clogit", "action_clogit", "seg_clogit")
ATTN_KEYS = ("a2f_attn", "f2a_attn_logit", "a2f_attn_logit")


def _np(t):
    return t.detach().cpu().numpy()


def make_cfg(spec):
    cfg = get_cfg_defaults()
    cfg.defrost()
    for sec in ("FACT", "Bi", "Bu", "BU", "Loss"):
        for k, v in spec.get(sec, {}).items():
            cfg[sec][k] = v
    cfg.TM.use = False
    return cfg


def video(v):
    return pg.segmented_video(v["T"], 40, v["classes"], v["nseg"], seed=v["seed"], noise=v["noise"])


def run_reference(spec, vids, dtype):
    """One forward + batch-mean loss + backward of the reference over ``vids`` in ``dtype``.  Returns
    (record, gradients); the record holds per video v: loss, pred, match, the segment bounds of every TDU
    block, the segmentation margins and the blended transcript probability (frames, N)."""
    torch.set_default_dtype(dtype)
    cfg = make_cfg(spec)
    net = rblocks.FACT(cfg, spec["D"], spec["C"])
    with torch.no_grad():
        for n, p in net.named_parameters():
            p.copy_(torch.from_numpy(pg.param_value(n, p.shape, spec["seed"])).to(dtype))
    net.mcriterion = rloss.MatchCriterion(cfg, spec["C"], [])
    rec = dict(match=[], segs=[], margin=[], blend=[])
    orig_match = net.mcriterion.match

    def match_spy(*a, **k):
        r = orig_match(*a, **k)
        rec["match"].append((_np(r[0]).astype(np.int64), _np(r[1]).astype(np.int64)))
        return r
    net.mcriterion.match = match_spy
    orig_down = rblocks.UpdateBlockTDU.temporal_downsample
    orig_eval = rblocks.Block._eval_w_transcript

    def down(self, frame_feature):
        top = torch.topk(frame_feature[:, 0, -self.nclass:].detach(), 2, dim=-1).values
        rec["margin"].append(float(((top[:, 0] - top[:, 1]) / top[:, 0]).min()))
        out = orig_down(self, frame_feature)
        rec["segs"].append((np.array([s.start for s in out[0].segs], dtype=np.int64),
                            np.array([s.end for s in out[0].segs], dtype=np.int64)))
        return out

    def ev(transcript, a2f_attn, frame_clogit, weight):
        # the reference's own expression (blocks.py:264-275), kept for the margin and the float32 spread
        fprob = torch.softmax(frame_clogit.squeeze(1), dim=-1)[:, transcript]
        aprob = torch.softmax(a2f_attn[0, :, :len(transcript)], dim=-1)
        rec["blend"].append(_np((1 - weight) * aprob + weight * fprob).astype(np.float64))
        return orig_eval(transcript, a2f_attn, frame_clogit, weight)
    rblocks.UpdateBlockTDU.temporal_downsample = down
    rblocks.Block._eval_w_transcript = staticmethod(ev)
    try:
        net.train()
        data = [video(v) for v in vids]
        total, saves = net([torch.from_numpy(f).to(dtype) for f, _ in data], [torch.from_numpy(l_) for _, l_ in data],
                           compute_loss=True)
        total.backward()
    finally:
        rblocks.UpdateBlockTDU.temporal_downsample = orig_down
        rblocks.Block._eval_w_transcript = staticmethod(orig_eval)
    nu = sum(1 for t in spec["FACT"]["block"] if t == "U")
    out = dict(total=float(total.item()), net=net, videos=[])
    for v in range(len(vids)):
        out["videos"].append(dict(loss=float(saves[v]["loss"]["loss"]), pred=np.asarray(saves[v]["pred"]).astype(np.int64),
                                  match=rec["match"][v], segs=rec["segs"][v * nu:(v + 1) * nu],
                                  margin=rec["margin"][v * nu:(v + 1) * nu], blend=rec["blend"][v],
                                  transcript=[int(c) for c in np.asarray(data[v][1])[
                                      np.r_[True, data[v][1][1:] != data[v][1][:-1]]]]))
    grads = {n: _np(p.grad).astype(np.float64) for n, p in net.named_parameters()}
    return out, grads


def pred_check(r64, r32):
    """Per video (relative top-2 margin of the blended probability, its largest relative f32-vs-f64 difference)."""
    out = []
    for a, b in zip(r64["videos"], r32["videos"]):
        top = -np.sort(-a["blend"], axis=1)[:, :2] if a["blend"].shape[1] > 1 else None
        margin = float(((top[:, 0] - top[:, 1]) / top[:, 0]).min()) if top is not None else float("inf")
        out.append((margin, float((np.abs(a["blend"] - b["blend"]) / np.abs(a["blend"])).max())))
    return out


def conditions(spec, vids, want_seg=MIN_SEG_MARGIN):
    """(ok, text) of the two fixture conditions for every video of ``vids`` under ``spec``."""
    r64, _ = run_reference(spec, vids, torch.float64)
    r32, _ = run_reference(spec, vids, torch.float32)
    torch.set_default_dtype(torch.float64)
    ok, lines = True, []
    for v, (rv, (pm, pd)) in enumerate(zip(r64["videos"], pred_check(r64, r32))):
        sm = min(rv["margin"])
        good = sm >= want_seg and pm >= PRED_MARGIN_FACTOR * pd and len(rv["transcript"]) == vids[v]["nseg"]
        ok = ok and good
        lines.append(f"  video T={vids[v]['T']} seed={vids[v]['seed']}: segmentation margin {sm:.3g}, prediction margin "
                     f"{pm:.3g} vs f32 difference {pd:.3g} (x{pm / max(pd, 1e-300):.0f}), TDU segments "
                     f"{[len(s[0]) for s in rv['segs']]}, loss {rv['loss']:.6f} -> {'ok' if good else 'FAILS'}")
    return ok, "\n".join(lines)


def find_seed(vid, prefer=2e-3, tries=40):
    """The first seed from vid['seed'] on for which the conditions hold under the iuU / sca / seq model (the
    only model B and C are used with) with a segmentation margin >= ``prefer``; failing that, the first for
    which they hold at all."""
    for want in (prefer, MIN_SEG_MARGIN):
        for seed in range(vid["seed"], vid["seed"] + tries):
            cand = dict(vid, seed=seed)
            if conditions(MODELS["sca"], [cand], want)[0]:
                return cand
    raise AssertionError(f"no seed in {tries} tries satisfies the fixture conditions for {vid}")


def videos():
    return VIDEO_A, VIDEO_B, VIDEO_C


def search():
    """The seed search that produced VIDEO_B / VIDEO_C; asserts that the recorded seeds are what it finds."""
    for name, vid in (("B", VIDEO_B), ("C", VIDEO_C)):
        found = find_seed(dict(vid, seed=SEARCH_FROM[name]))
        print(name, "seed", found["seed"])
        assert found["seed"] == vid["seed"], (name, found["seed"], vid["seed"])


def _record_single(spec, vid, r, grads):
    from make_golden import grad_record
    net, rv = r["net"], r["videos"][0]
    out = {"T": vid["T"], "D": spec["D"], "C": spec["C"]}
    out["loss"] = np.array([r["total"]])
    out["pred"], out["match_a"], out["match_s"] = rv["pred"], rv["match"][0], rv["match"][1]
    out["transcript"] = np.array(rv["transcript"], dtype=np.int64)
    out["frame_pe"] = _np(net.frame_pe.pe[:vid["T"], 0])
    out["action_pe"] = _np(net.action_pe.pe[:len(rv["transcript"]), 0])
    for i, blk in enumerate(net.block_list):
        p = f"block{i}/"
        for k in SIDE_KEYS:
            if hasattr(blk, k):
                out[p + k] = _np(getattr(blk, k)[:, 0])
        for k in ATTN_KEYS:
            if getattr(blk, k, None) is not None:
                out[p + k] = _np(getattr(blk, k)[0])
        if hasattr(blk, "tdu"):
            out[p + "seg_start"] = np.array([s.start for s in blk.tdu.segs], dtype=np.int64)
            out[p + "seg_end"] = np.array([s.end for s in blk.tdu.segs], dtype=np.int64)
    for n, g in grads.items():
        grad_record("", n, torch.from_numpy(g), out, full_limit=16384, dtype=np.float64)
    meta = dict(spec, video=vid, T=vid["T"], nseg=vid["nseg"], noise=vid["noise"], seen=vid["classes"])
    meta["param_shapes"] = {n: list(p.shape) for n, p in net.named_parameters()}
    meta["nullw"] = spec["Loss"]["nullw"]
    meta["min_margin"] = min(rv["margin"])
    out["meta_json"] = np.array(json.dumps(meta))
    return out


def capture():
    from make_golden import grad_record
    A, B, C = videos()
    for spec, vids in ((MODELS["sca"], [A, B, C]), (MODELS["gru"], [A])):
        ok, text = conditions(spec, vids)
        print(spec["FACT"]["block"], spec["Bi"]["a"], spec["Loss"]["match"])
        print(text)
        assert ok, "fixture conditions violated; pick other seeds"
    # tiny_trans, tiny_trans_gru: video A alone
    for name, key in (("tiny_trans", "sca"), ("tiny_trans_gru", "gru")):
        spec = MODELS[key]
        r, grads = run_reference(spec, [A], torch.float64)
        out = _record_single(spec, A, r, grads)
        n = save_fixture(name, out)
        print(f"{name}: {n} part(s), loss {r['total']:.6f}, transcript {r['videos'][0]['transcript']}, TDU segments "
              f"{[len(s[0]) for s in r['videos'][0]['segs']]}, match {r['videos'][0]['match'][0].tolist()}")
    # tiny_trans_batch: [A, B] (one pass) and [A, B, C] (three passes)
    spec = MODELS["sca"]
    out = {}
    for tag, vids in (("ab", [A, B]), ("abc", [A, B, C])):
        r, grads = run_reference(spec, vids, torch.float64)
        out[f"{tag}/loss"] = np.array([r["total"]])
        out[f"{tag}/video_loss"] = np.array([rv["loss"] for rv in r["videos"]])
        for v, rv in enumerate(r["videos"]):
            p = f"{tag}/vid{v}/"
            out[p + "pred"] = rv["pred"]
            out[p + "transcript"] = np.array(rv["transcript"], dtype=np.int64)
            for i, (st, en) in enumerate(rv["segs"]):
                out[p + f"tdu{i}/seg_start"], out[p + f"tdu{i}/seg_end"] = st, en
        for n, g in grads.items():
            grad_record(tag + "/", n, torch.from_numpy(g), out, full_limit=16384, dtype=np.float64)
        print(f"tiny_trans_batch {tag}: loss {r['total']:.6f}, per video {[round(rv['loss'], 6) for rv in r['videos']]}")
    meta = dict(spec, videos=[A, B, C])
    meta["param_shapes"] = {n: list(p.shape) for n, p in r["net"].named_parameters()}
    meta["nullw"] = spec["Loss"]["nullw"]
    out["meta_json"] = np.array(json.dumps(meta))
    print("tiny_trans_batch:", save_fixture("tiny_trans_batch", out), "part(s)")


def spread():
    """The reference in float32 against its float64 run, per compared quantity and case."""
    A, B, C = videos()
    for name, spec, vids in (("tiny_trans", MODELS["sca"], [A]), ("tiny_trans_batch [A, B]", MODELS["sca"], [A, B]),
                             ("tiny_trans_batch [A, B, C]", MODELS["sca"], [A, B, C]),
                             ("tiny_trans_gru", MODELS["gru"], [A])):
        r64, g64 = run_reference(spec, vids, torch.float64)
        r32, g32 = run_reference(spec, vids, torch.float32)
        torch.set_default_dtype(torch.float64)
        print(name)
        for a, b in zip(r64["videos"], r32["videos"]):
            assert np.array_equal(a["pred"], b["pred"]) and all(np.array_equal(x, y) for x, y in zip(a["match"], b["match"]))
            assert all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a["segs"], b["segs"]))
        print("  pred, match, segment bounds: equal")
        rel = max([abs(r32["total"] - r64["total"]) / abs(r64["total"])] +
                  [abs(b["loss"] - a["loss"]) / abs(a["loss"]) for a, b in zip(r64["videos"], r32["videos"])])
        print(f"  loss (relative, batch and per video)                         {rel:.3g}   bound 2e-5")
        if len(vids) == 1:
            worst = {}
            for i, (b64, b32) in enumerate(zip(r64["net"].block_list, r32["net"].block_list)):
                for k in SIDE_KEYS + ATTN_KEYS:
                    if getattr(b64, k, None) is not None:
                        d = float((_np(getattr(b64, k)) - _np(getattr(b32, k)).astype(np.float64)).__abs__().max())
                        worst[k] = max(worst.get(k, 0.0), d)
            for k, v in worst.items():
                print(f"  {k:60s} {v:.3g}   bound 1e-4 + 1e-4 |ref|")
        ratio, who = 0.0, None
        for n, r in g64.items():
            r = r.reshape(-1)
            g = g32[n].reshape(-1)
            rms = float(np.sqrt((r * r).mean()))
            q = float((np.abs(g - r) / (2e-3 * np.abs(r) + 2e-3 * rms + 1e-6)).max())
            if q > ratio:
                ratio, who = q, n
        print(f"  gradients (fraction of rtol 2e-3 + 2e-3 RMS + 1e-6)           {ratio:.3g}   ({who})")
        for (pm, pd), v in zip(pred_check(r64, r32), vids):
            print(f"  prediction margin T={v['T']}: {pm:.3g}, f32 difference {pd:.3g}")


if __name__ == "__main__":
    if "--search" in sys.argv[1:]:
        search()
    elif "--spread" in sys.argv[1:]:
        spread()
    else:
        capture()
