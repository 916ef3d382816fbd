"""Capture the ``tiny_vn`` golden fixture from the reference's verb/noun FACT
(fact_clip/models/blocks_SepVerbNoun.py; build container only, like make_golden.py).

Run:  python tests/golden/make_golden_vn.py            # writes tiny_vn.<i>.npz
      python tests/golden/make_golden_vn.py --spread   # the reference in float32 vs its float64 run

The mapping is synthetic (5 verbs, 7 nouns, 12 actions: distinct pairs that reach the last verb
and the last noun) and is assigned to the reference's module globals before construction, so no
``data/`` files are read.  Weights and inputs come from ``paramgen``; the fixture stores expected
outputs and gradients in the layout ``helpers.cfg_from_meta`` / ``check_grad`` read.

Margin condition: at every TDU segmentation the combined action probability's relative top-2 margin
must be >= 1e-3 on every frame (asserted), so that an fp32 argmax cannot move a segment boundary.

``--spread`` measures how far the reference's own float32 run sits from its float64 run for every
quantity the GPU test compares; tests/test_gpu_verbnoun.py derives its tolerances from those numbers
(DESIGN.md section 7l).
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
from fact_clip.models import loss as rloss  # noqa: E402
from fact_clip.models import blocks_SepVerbNoun as vn  # noqa: E402

MIN_MARGIN = 1e-3

VIDS = [0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 0, 2]
NIDS = [0, 1, 2, 3, 4, 5, 6, 0, 1, 2, 3, 6]

SPEC = dict(model="FACT_VN", T=150, D=40, C=12, V=5, N=7, nseg=4, noise=0.3, seed=1,
            FACT=dict(ntoken=8, block="IUU", fpos=True, cmr=0.0, mwt=0.1, trans=False),
            Bi=dict(hid_dim=48, dropout=0.0, a="sca", a_nhead=4, a_ffdim=48, a_layers=2, a_dim=32,
                    f="m", f_layers=3, f_ln=False, f_dim=24, f_ngp=1),
            BU=dict(f_layers=3, a_nhead=4, s_layers=1),
            Loss=dict(pc=0.2, a2fc=1.0, match="o2o", bgw=1.0, sw=5.0),
            holdout=[])

BLOCK_KEYS = ("frame_logp", "seg_logp", "action_logp")
ATTN_KEYS = ("a2f_attn", "f2a_attn_logit", "a2f_attn_logit")


def _np(t):
    return t.detach().cpu().numpy()


def make_cfg(spec):
    cfg = get_cfg_defaults()
    cfg.defrost()
    for sec in ("FACT", "Bi", "BU", "Loss"):
        for k, v in spec.get(sec, {}).items():
            cfg[sec][k] = v
    cfg.TM.use = False
    Q = spec["FACT"]["ntoken"]
    cfg.Loss.nullw = Q / ((Q - spec["nseg"]) * spec["C"])
    return cfg


def run_reference(spec, dtype):
    """One forward + loss + backward of the reference model in ``dtype``; returns a flat record."""
    torch.set_default_dtype(dtype)
    vn._VIDS, vn._NIDS = list(VIDS), list(NIDS)
    cfg = make_cfg(spec)
    T, D, C, seed = spec["T"], spec["D"], spec["C"], spec["seed"]
    feats, label = pg.segmented_video(T, D, list(range(C)), spec["nseg"], seed=seed, noise=spec["noise"])
    net = vn.FACT(cfg, D, spec["V"], spec["N"])
    with torch.no_grad():
        for n, p in net.named_parameters():
            p.copy_(torch.from_numpy(pg.param_value(n, p.shape, seed)).to(dtype))
    net.mcriterion = rloss.MatchCriterion(cfg, C, [])
    rec = {"margin": []}
    orig_match = net.mcriterion.match

    def spy(*a, **k):
        r = orig_match(*a, **k)
        rec["match"] = r
        return r
    net.mcriterion.match = spy

    # the margin of every segmentation argmax (the reference's own expression, blocks_SepVerbNoun.py:287-292)
    orig_down = vn.Block.temporal_downsample

    def down(self, frame_feature):
        cprob = frame_feature[..., -self.nclass1 - self.nclass2:]
        vprob, nprob = cprob[..., :self.nclass1], cprob[..., self.nclass1:]
        top = torch.topk((vprob[..., vn._VIDS] * nprob[..., vn._NIDS])[:, 0].detach(), 2, dim=-1).values
        rec["margin"].append(float(((top[:, 0] - top[:, 1]) / top[:, 0]).min()))
        return orig_down(self, frame_feature)
    vn.Block.temporal_downsample = down
    try:
        net.train()
        total, saves = net([torch.from_numpy(feats).to(dtype)], [torch.from_numpy(label)], compute_loss=True)
        total.backward()
    finally:
        vn.Block.temporal_downsample = orig_down

    out = {"T": T, "D": D, "C": C}
    out["loss"] = np.array([total.item()])
    out["pred"] = saves[0]["pred"].astype(np.int64)
    out["match_a"] = _np(rec["match"][0]).astype(np.int64)
    out["match_s"] = _np(rec["match"][1]).astype(np.int64)
    out["vids"] = np.array(VIDS, dtype=np.int64)
    out["nids"] = np.array(NIDS, dtype=np.int64)
    out["frame_pe"] = _np(net.frame_pe.pe[:T, 0])
    for i, blk in enumerate(net.block_list):
        p = f"block{i}/"
        for k in BLOCK_KEYS:
            out[p + k] = _np(getattr(blk, k)[:, 0])
        for k in ATTN_KEYS:
            if getattr(blk, k, None) is not None:
                out[p + k] = _np(getattr(blk, k)[0])
        out[p + "seg_start"] = np.array([s.start for s in blk.tdu.segs], dtype=np.int64)
        out[p + "seg_end"] = np.array([s.end for s in blk.tdu.segs], dtype=np.int64)
    grads = {n: _np(p.grad).astype(np.float64) for n, p in net.named_parameters()}
    assert all(g is not None for g in grads.values())
    meta = dict(spec)
    meta["param_shapes"] = {n: list(p.shape) for n, p in net.named_parameters()}
    meta["nullw"] = cfg.Loss.nullw
    meta["seen"] = list(range(C))
    return out, grads, meta, rec["margin"]


def capture():
    from make_golden import grad_record
    out, grads, meta, margins = run_reference(SPEC, torch.float64)
    print("top-2 margins per TDU segmentation:", ["%.3g" % m for m in margins])
    assert min(margins) >= MIN_MARGIN, f"margin condition violated: {margins}; pick another seed"
    for n, g in grads.items():
        grad_record("", n, torch.from_numpy(g), out, full_limit=16384, dtype=np.float64)
    meta["min_margin"] = min(margins)
    out["meta_json"] = np.array(json.dumps(meta))
    nparts = save_fixture("tiny_vn", out)
    print("tiny_vn:", nparts, "part(s), loss", out["loss"][0], "segments per block",
          [len(out[f"block{i}/seg_start"]) for i in range(len(SPEC["FACT"]["block"]))], "params", len(grads))


def spread():
    """The reference in float32 against its float64 run, per compared quantity."""
    o64, g64, _, _ = run_reference(SPEC, torch.float64)
    o32, g32, _, _ = run_reference(SPEC, torch.float32)
    torch.set_default_dtype(torch.float64)
    worst = {}
    for k in o64:
        if not k.startswith("block"):
            continue
        name = k.split("/")[1]
        if name in ("seg_start", "seg_end"):
            assert np.array_equal(o64[k], o32[k]), k
            continue
        worst[name] = max(worst.get(name, 0.0), float(np.abs(o64[k] - o32[k]).max()))
    for k in ("pred", "match_a", "match_s"):
        assert np.array_equal(o64[k], o32[k]), k
    worst["loss (relative)"] = abs(o32["loss"][0] - o64["loss"][0]) / abs(o64["loss"][0])
    ratio, who = 0.0, None
    for n, r in g64.items():
        r = r.reshape(-1)
        g = g32[n].reshape(-1)
        rms = float(np.sqrt((r * r).mean()))
        tol = 2e-3 * np.abs(r) + 2e-3 * rms + 1e-6          # test_gpu_parity's gradient bound
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
