"""Device time and peak memory of the verb/noun model's per-video loss phase and prediction:
the fused path (functional.vn_class_loss / vn_eval_pred, no T x A table) against the eager path on
the materialised action log-probabilities (verb_noun_logp + the ``is_logit=False`` terms of
models/loss.py + Block.action_token_loss + Block._eval).

python tools/vn_loss_time.py [--iters 20] [--rounds 3] [--out profiles/vn_loss.json] [--commit HASH]

Two shapes: the ``tiny_vn`` fixture's (T = 150, 5 / 7 heads, 12 actions, 8 tokens, 40 segments) and
an EPIC-like one (T = 4096, 98 / 301 heads, 4000 actions, 300 tokens, 100 segments).  The timed work
of the loss phase is one block's forward terms (frame + segment + smooth + token) plus the backward
into the three class-logit tensors; of the prediction, one call.  HIP events around single calls after
a warm-up, fixed seeds; each figure is the median of --iters calls, and the two paths alternate
--rounds times in one run so the spread of the repeats is seen next to the difference.  Peak memory is
torch.cuda.max_memory_allocated over one call, above what is allocated before it.  Prints one JSON
object, and writes it to --out.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fact-clip_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from factmx import functional as fxf  # noqa: E402
from factmx.configs import get_cfg_defaults  # noqa: E402
from factmx.models import loss as L  # noqa: E402
from factmx.models.basic import TemporalDownsampleUpsample  # noqa: E402
from factmx.models.blocks_SepVerbNoun import Block  # noqa: E402
from factmx.models.loss import MatchCriterion  # noqa: E402

DEV = "cuda"
SHAPES = {"tiny_vn": dict(T=150, V=5, N=7, A=12, Q=8, S=40, G=6),
          "epic_like": dict(T=4096, V=98, N=301, A=4000, Q=300, S=100, G=60)}
SW, MWT = 5.0, 0.3


def make_case(T, V, N, A, Q, S, G, seed=0):
    """Class logits of one block, G ground-truth segments, S TDU segments, a one-to-one match."""
    rng = np.random.default_rng(seed)
    vids, nids = rng.integers(0, V, A), rng.integers(0, N, A)
    vids[-1], nids[-1] = V - 1, N - 1
    m = fxf.VerbNounMap(vids.tolist(), nids.tolist())
    gen = torch.Generator().manual_seed(seed)
    cl = [torch.randn(r, c, generator=gen).to(DEV) for r, c in ((T, V + N), (S, V + N), (Q, V + N + 2))]
    cuts = np.sort(rng.choice(np.arange(1, T), G - 1, replace=False))
    label = np.repeat(rng.integers(0, A, G), np.diff(np.concatenate([[0], cuts, [T]])))
    tcuts = np.concatenate([[0], np.sort(rng.choice(np.arange(1, T), S - 1, replace=False)), [T]])
    st, en = torch.from_numpy(tcuts[:-1]).to(torch.int32), torch.from_numpy(tcuts[1:] - 1).to(torch.int32)
    sid = torch.from_numpy(np.repeat(np.arange(S), np.diff(tcuts))).to(torch.int32)
    tdu = TemporalDownsampleUpsample(sid.to(DEV), st.to(DEV), en.to(DEV))
    cfg = get_cfg_defaults()
    crit = MatchCriterion(cfg, A, [])
    crit.set_label(torch.from_numpy(label).to(DEV))
    nseg = int(crit.transcript.shape[0])
    k = min(Q, nseg)
    match = (torch.from_numpy(rng.permutation(Q)[:k].copy()), torch.from_numpy(rng.permutation(nseg)[:k].copy()))
    attn = torch.softmax(torch.randn(T, Q, generator=gen), -1).to(DEV).unsqueeze(0)
    m.tables(DEV), m.csr(DEV, V, N), m.csr(DEV, V + 1, N + 1)
    return dict(m=m, cl=cl, tdu=tdu, crit=crit, match=match, attn=attn)


def fused_loss(c):
    f, s, a = (x.detach().requires_grad_(True) for x in c["cl"])
    crit, m = c["crit"], c["m"]
    lo = (crit.vn_frame_terms(f, m, ce_coef=0.25, sm_coef=SW) + crit.vn_seg_terms(s, m, c["tdu"], ce_coef=0.25)
          + crit.vn_token_terms(c["match"], a, m, 0.5))
    lo.backward()
    return lo, (f.grad, s.grad, a.grad)


def eager_loss(c):
    f, s, a = (x.detach().requires_grad_(True) for x in c["cl"])
    crit, m = c["crit"], c["m"]
    flp = fxf.verb_noun_logp(f, m).unsqueeze(1)
    slp = fxf.verb_noun_logp(s, m).unsqueeze(1)
    alp = fxf.verb_noun_logp(a, m, action=True).unsqueeze(1)
    fl = crit.frame_loss(flp.squeeze(1), is_logit=False) / 2
    sl = crit.frame_loss_tdu(slp, c["tdu"], is_logit=False) / 2
    sm = L.smooth_loss(torch.transpose(flp, 0, 1), is_logit=False)
    lo = (fl + sl) / 2 + SW * sm + Block.action_token_loss(None, crit, c["match"], alp) / 2
    lo.backward()
    return lo, (f.grad, s.grad, a.grad)


def fused_pred(c):
    return fxf.vn_eval_pred(c["cl"][2], c["cl"][0], c["attn"], c["m"], MWT)


def eager_pred(c):
    with torch.no_grad():
        return Block._eval(fxf.verb_noun_logp(c["cl"][2], c["m"], action=True).unsqueeze(1), c["attn"],
                           fxf.verb_noun_logp(c["cl"][0], c["m"]).unsqueeze(1), MWT)


def timed(fn, c, iters, warmup=3):
    for _ in range(warmup):
        fn(c)
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(c)
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return round(statistics.median(ts), 1)


def peak(fn, c):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    r = fn(c)
    torch.cuda.synchronize()
    del r
    return round((torch.cuda.max_memory_allocated() - base) / 1e6, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vn_loss.json"))
    ap.add_argument("--commit", default=None, help="commit hash of the code under test, recorded in the output")
    args = ap.parse_args()
    res = {"commit": args.commit, "device": torch.cuda.get_device_name(0), "iters": args.iters,
           "unit": "median microseconds per call (event-timed, host launch work included); peak MB above the inputs",
           "shapes": {}}
    for name, shp in SHAPES.items():
        c = make_case(**shp)
        lf, gf = fused_loss(c)
        le, ge = eager_loss(c)
        out = dict(shp, table_MB=round(shp["T"] * shp["A"] * 4 / 1e6, 2),
                   loss_fused=float(lf.detach()), loss_eager=float(le.detach()),
                   grad_max_diff=max(float((a - b).abs().max()) for a, b in zip(gf, ge)),
                   pred_equal=bool(torch.equal(fused_pred(c), eager_pred(c))))
        c["crit"].onehot_class_label = None          # (the eager run built it: measure the fused path without it)
        for key, fn in (("loss_fused", fused_loss), ("loss_eager", eager_loss), ("pred_fused", fused_pred),
                        ("pred_eager", eager_pred)):
            out[key + "_peak_MB"] = peak(fn, c)
            if key == "loss_eager":
                c["crit"].onehot_class_label = None
        for key in ("loss_fused", "loss_eager", "pred_fused", "pred_eager"):
            out[key + "_us"] = []
        for _ in range(args.rounds):                 # the two paths alternate
            for key, fn in (("loss_fused", fused_loss), ("loss_eager", eager_loss), ("pred_fused", fused_pred),
                            ("pred_eager", eager_pred)):
                out[key + "_us"].append(timed(fn, c, args.iters))
        res["shapes"][name] = out
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
