"""Capture the ``tiny_vn_o2m`` golden fixture from the reference's verb/noun FACT with one-to-many
matching (fact_clip/models/blocks_SepVerbNoun.py, loss.py:155-193; build container only).

Run:  python tests/golden/make_golden_vn_o2m.py        # writes tiny_vn_o2m.<i>.npz

The machinery is make_golden_vn.py's (same synthetic mapping, paramgen weights and inputs, record
layout); the settings differ: ``match: o2m``, 16 tokens, T = 300 frames in 72 ground-truth segments, so
every loss term of the update blocks works on K = 72 > 64 matched columns with repeated tokens.

Conditions asserted on the reference's own float64 run:
  * the segmentation margin of make_golden_vn.py at every TDU segmentation (>= 1e-3);
  * the match is stable: moving every entry of the reference's cost matrix by +- 2e-5 x (1 + max|cost|)
    (two seeded sign patterns) gives the same one-to-many pairs, so an fp32 cost cannot change them.
"""
import json
import sys

import numpy as np

import make_golden_vn as base          # (sets up sys.path and imports the reference)

torch = base.torch
rloss = base.rloss

BOUND = 2e-5

SPEC = dict(model="FACT_VN", T=300, D=40, C=12, V=5, N=7, nseg=72, noise=0.3, seed=4,
            FACT=dict(ntoken=16, block="IUU", fpos=True, cmr=0.0, mwt=0.1, trans=False),
            Bi=dict(hid_dim=48, dropout=0.0, a="sca", a_nhead=4, a_ffdim=48, a_layers=2, a_dim=32,
                    f="m", f_layers=3, f_ln=False, f_dim=24, f_ngp=1),
            BU=dict(f_layers=3, a_nhead=4, s_layers=1),
            Loss=dict(pc=0.2, a2fc=1.0, match="o2m", bgw=1.0, sw=5.0),
            holdout=[])
NULLW = 0.1


def _make_cfg(spec, _orig=base.make_cfg):
    cfg = _orig(spec)
    cfg.Loss.nullw = NULLW            # (make_golden_vn's rule counts one token per segment: o2o only)
    return cfg


def capture():
    from make_golden import grad_record
    costs = []
    orig = rloss.MatchCriterion._one_to_many_match

    def spy(self, cost):
        costs.append((self, np.array(cost, dtype=np.float64)))
        return orig(self, cost)
    base.make_cfg = _make_cfg
    rloss.MatchCriterion._one_to_many_match = spy
    try:
        out, grads, meta, margins = base.run_reference(SPEC, torch.float64)
    finally:
        rloss.MatchCriterion._one_to_many_match = orig
    print("top-2 margins per TDU segmentation:", ["%.3g" % m for m in margins])
    assert min(margins) >= base.MIN_MARGIN, f"margin condition violated: {margins}; pick another seed"
    assert len(costs) == 1
    crit, cost = costs[0]
    want = orig(crit, cost)
    lim = BOUND * (1.0 + float(np.abs(cost).max()))
    for seed in (1, 2):
        sign = np.where(np.random.default_rng(seed).random(cost.shape) < 0.5, -1.0, 1.0)
        assert orig(crit, cost + lim * sign) == want, "the match sits on a near-tie; pick another seed"
    K = len(out["match_a"])
    assert K == SPEC["nseg"] > 64 and len(set(out["match_a"].tolist())) < K
    for n, g in grads.items():
        grad_record("", n, torch.from_numpy(g), out, full_limit=16384, dtype=np.float64)
    meta["min_margin"] = min(margins)
    out["meta_json"] = np.array(json.dumps(meta))
    nparts = base.save_fixture("tiny_vn_o2m", out)
    print("tiny_vn_o2m:", nparts, "part(s), loss", out["loss"][0], "K", K, "segments per block",
          [len(out[f"block{i}/seg_start"]) for i in range(len(SPEC["FACT"]["block"]))], "params", len(grads))


if __name__ == "__main__":
    sys.exit(capture())
