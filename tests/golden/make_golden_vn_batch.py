"""Capture the ``tiny_vn_batch`` golden fixture: one step of the reference's verb/noun FACT
(fact_clip/models/blocks_SepVerbNoun.py; build container only) over THREE ragged videos.

Run:  python tests/golden/make_golden_vn_batch.py            # writes tiny_vn_batch.<i>.npz
      python tests/golden/make_golden_vn_batch.py --spread   # the reference in float32 vs its float64 run

The machinery is make_golden_vn.py's (same synthetic mapping, configuration, paramgen weights of seed 1,
record layout); the step is one ``forward(seq_list, label_list, compute_loss=True)`` + backward of the batch
loss (the mean of the per-video losses) in float64.  The fixture records the batch loss, per video its
loss, prediction, match and per-block TDU segment bounds, and the gradients of the batch loss.

Conditions asserted on the reference's own float64 run, for every video:
  * the segmentation margin of make_golden_vn.py at every TDU segmentation (>= 1e-3);
  * the match is stable: moving every entry of the video's cost matrix by +- 2e-5 x (1 + max|cost|)
    (two seeded sign patterns, as make_golden_vn_o2m.py) gives the same pairs.
"""
import json
import sys

import numpy as np

import make_golden_vn as base          # (sets up sys.path and imports the reference)

torch = base.torch
rloss = base.rloss
vn = base.vn
pg = base.pg

BOUND = 2e-5
# (T, nseg, seed) of pg.segmented_video(T, 40, range(12), nseg, seed, noise=0.3)
VIDEOS = [(150, 4, 1), (97, 3, 3), (211, 5, 2)]
SPEC = dict(base.SPEC, videos=[list(v) for v in VIDEOS])


def make_videos(spec):
    return [pg.segmented_video(T, spec["D"], list(range(spec["C"])), nseg, seed=seed, noise=spec["noise"])
            for T, nseg, seed in spec["videos"]]


def run_reference(spec, dtype):
    """One forward + loss + backward of the reference over the batch in ``dtype``: a flat record, the
    gradients, the meta data, per video the margins of its segmentations and its cost matrix."""
    torch.set_default_dtype(dtype)
    vn._VIDS, vn._NIDS = list(base.VIDS), list(base.NIDS)
    cfg = base.make_cfg(spec)           # (nullw from tiny_vn's nseg: its configuration as it is)
    D, C, seed = spec["D"], spec["C"], spec["seed"]
    vids = make_videos(spec)
    net = vn.FACT(cfg, D, spec["V"], spec["N"])
    with torch.no_grad():
        for n, p in net.named_parameters():
            p.copy_(torch.from_numpy(pg.param_value(n, p.shape, seed)).to(dtype))
    net.mcriterion = rloss.MatchCriterion(cfg, C, [])
    margins, matches, costs, bounds = [[]], [], [], []

    orig_match = net.mcriterion.match

    def match_spy(*a, **k):
        r = orig_match(*a, **k)
        matches.append(r)
        return r
    net.mcriterion.match = match_spy

    orig_lsa = rloss.linear_sum_assignment

    def lsa_spy(cost):
        costs.append(np.array(cost, dtype=np.float64))
        return orig_lsa(cost)
    rloss.linear_sum_assignment = lsa_spy

    orig_down = vn.Block.temporal_downsample

    def down(self, frame_feature):
        cprob = frame_feature[..., -self.nclass1 - self.nclass2:]
        vprob, nprob = cprob[..., :self.nclass1], cprob[..., self.nclass1:]
        top = torch.topk((vprob[..., vn._VIDS] * nprob[..., vn._NIDS])[:, 0].detach(), 2, dim=-1).values
        margins[-1].append(float(((top[:, 0] - top[:, 1]) / top[:, 0]).min()))
        return orig_down(self, frame_feature)
    vn.Block.temporal_downsample = down

    orig_loss = net._loss_one_video

    def loss_spy(label):          # after each video's forward: its segmentations are still on the blocks
        bounds.append([(np.array([s.start for s in blk.tdu.segs], dtype=np.int64),
                        np.array([s.end for s in blk.tdu.segs], dtype=np.int64)) for blk in net.block_list])
        margins.append([])
        return orig_loss(label)
    net._loss_one_video = loss_spy
    try:
        net.train()
        total, saves = net([torch.from_numpy(f).to(dtype) for f, _ in vids], [torch.from_numpy(l_) for _, l_ in vids],
                           compute_loss=True)
        total.backward()
    finally:
        vn.Block.temporal_downsample = orig_down
        rloss.linear_sum_assignment = orig_lsa
    margins = margins[:len(vids)]
    assert len(matches) == len(costs) == len(bounds) == len(vids)

    out = {"D": D, "C": C, "nvid": len(vids)}
    out["loss"] = np.array([total.item()])
    out["vids"] = np.array(base.VIDS, dtype=np.int64)
    out["nids"] = np.array(base.NIDS, dtype=np.int64)
    for v, save in enumerate(saves):
        p = f"video{v}/"
        out[p + "loss"] = np.array([save["loss"]["loss"]])
        out[p + "pred"] = save["pred"].astype(np.int64)
        out[p + "match_a"] = base._np(matches[v][0]).astype(np.int64)
        out[p + "match_s"] = base._np(matches[v][1]).astype(np.int64)
        for k, (st, en) in enumerate(bounds[v]):
            out[p + f"block{k}/seg_start"] = st
            out[p + f"block{k}/seg_end"] = en
    grads = {n: base._np(p.grad).astype(np.float64) for n, p in net.named_parameters()}
    meta = dict(spec)
    meta["param_shapes"] = {n: list(p.shape) for n, p in net.named_parameters()}
    meta["nullw"] = cfg.Loss.nullw
    meta["seen"] = list(range(C))
    return out, grads, meta, margins, costs


def capture():
    from make_golden import grad_record
    out, grads, meta, margins, costs = run_reference(SPEC, torch.float64)
    for v, (m, cost) in enumerate(zip(margins, costs)):
        print(f"video {v} {tuple(SPEC['videos'][v])}: top-2 margins", ["%.3g" % x for x in m], "segments per block",
              [len(out[f"video{v}/block{k}/seg_start"]) for k in range(len(SPEC["FACT"]["block"]))])
        assert min(m) >= base.MIN_MARGIN, f"video {v}: margin condition violated: {m}; swap the video"
        want = rloss.linear_sum_assignment(cost)
        lim = BOUND * (1.0 + float(np.abs(cost).max()))
        for seed in (1, 2):
            sign = np.where(np.random.default_rng(seed).random(cost.shape) < 0.5, -1.0, 1.0)
            got = rloss.linear_sum_assignment(cost + lim * sign)
            assert all(np.array_equal(a, b) for a, b in zip(got, want)), \
                f"video {v}: the match sits on a near-tie; swap the video"
    for n, g in grads.items():
        grad_record("", n, torch.from_numpy(g), out, full_limit=16384, dtype=np.float64)
    meta["min_margin"] = min(min(m) for m in margins)
    out["meta_json"] = np.array(json.dumps(meta))
    import fixture_io
    fixture_io.PART_BYTES = 700 * 1024          # every part smaller than tiny_vn's
    nparts = base.save_fixture("tiny_vn_batch", out)
    print("tiny_vn_batch:", nparts, "part(s), batch loss", out["loss"][0], "video losses",
          [float(out[f"video{v}/loss"][0]) for v in range(len(VIDEOS))], "params", len(grads))


def spread():
    """The reference in float32 against its float64 run on this batch, per compared quantity."""
    o64, g64, _, _, _ = run_reference(SPEC, torch.float64)
    o32, g32, _, _, _ = run_reference(SPEC, torch.float32)
    torch.set_default_dtype(torch.float64)
    worst = {"batch loss (relative)": abs(o32["loss"][0] - o64["loss"][0]) / abs(o64["loss"][0])}
    for k in o64:
        if not k.startswith("video"):
            continue
        if k.endswith("/loss"):
            worst["video loss (relative)"] = max(worst.get("video loss (relative)", 0.0),
                                                 abs(o32[k][0] - o64[k][0]) / abs(o64[k][0]))
        else:                       # predictions, matches, segment bounds
            assert np.array_equal(o64[k], o32[k]), k
    ratio, who = 0.0, None
    for n, r in g64.items():
        r = r.reshape(-1)
        g = g32[n].reshape(-1)
        rms = float(np.sqrt((r * r).mean()))
        tol = 2e-3 * np.abs(r) + 2e-3 * rms + 1e-6          # the gradient bound of the GPU tests
        q = float((np.abs(g - r) / tol).max())
        if q > ratio:
            ratio, who = q, n
    worst["gradients (fraction of rtol 2e-3 + 2e-3 RMS + 1e-6)"] = ratio
    for k, v in worst.items():
        print(f"{k:60s} {v:.3g}")
    print("worst gradient:", who)


if __name__ == "__main__":
    if "--spread" in sys.argv[1:]:
        spread()
    else:
        capture()
