"""Time and peak memory of the verb/noun model's loss phase of one video -- the matching, every loss
term forward, and the backward into the class and attention logits -- with the one-table path
(models/vn_vloss.py: fx_vn_match_cost, one fx_loss_terms_fwd / _bwd) against ``FUSED_TABLE = False``
(the per-term path: the eager soft-IoU cube, one launch pair per class term, eager cross-attention
terms).

python tools/vn_step_time.py [--iters 20] [--rounds 3] [--out profiles/vn_table.json] [--commit HASH]

Two shapes: the ``tiny_vn`` fixture's (T = 150, 5 / 7 heads, 12 actions, 8 tokens, 40 TDU segments, 6
ground-truth segments, IUU, o2o) and an EPIC-like one (T = 4096, 98 / 301 heads, 4000 actions, 300 tokens,
100 TDU segments, 130 ground-truth segments, IUUU, o2m).  A FACT of small feature widths is built for its
blocks' loss code only; no forward runs: every block gets synthetic class logits, attention logits and
TDU intervals of the shape's sizes as leaf tensors, and the timed call is FACT._loss_one_video plus the
backward of its result.  What the forward of either path leaves behind is made before the clock starts
(``action_logp``; for the per-term path also the frame-level ``a2f_attn``, which the parent commit's
forward stored).  HIP events around single calls after a warm-up (host work -- the Hungarian matching,
launches -- is inside the interval); each figure is the median of --iters calls and the two paths
alternate --rounds times.  Peak memory is torch.cuda.max_memory_allocated over one call above what is
allocated before it.  Prints one JSON object and writes it to --out.
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

from factmx.configs import get_cfg_defaults  # noqa: E402
from factmx.models import blocks_SepVerbNoun as vn  # noqa: E402
from factmx.models import vn_vloss  # noqa: E402
from factmx.models.basic import TemporalDownsampleUpsample  # noqa: E402
from factmx.models.loss import MatchCriterion  # noqa: E402

DEV = "cuda"
SHAPES = {"tiny_vn": dict(T=150, V=5, N=7, A=12, Q=8, S=40, G=6, block="IUU", match="o2o"),
          "epic_like": dict(T=4096, V=98, N=301, A=4000, Q=300, S=100, G=130, block="IUUU", match="o2m")}


def make_case(T, V, N, A, Q, S, G, block, match, seed=0):
    rng = np.random.default_rng(seed)
    vids, nids = rng.integers(0, V, A), rng.integers(0, N, A)
    vids[-1], nids[-1] = V - 1, N - 1
    m = vn.set_verb_noun_ids(vids.tolist(), nids.tolist())
    cfg = get_cfg_defaults()
    cfg.Bi.update(dict(hid_dim=32, a_dim=32, f_dim=32, a_ffdim=32, a_nhead=4, f_layers=2, a_layers=1, dropout=0.0, f="m",
                       a="sca", f_ln=False, f_ngp=1))
    cfg.BU.update(dict(f_layers=2, a_nhead=4, s_layers=1))
    cfg.FACT.update(dict(ntoken=Q, block=block, cmr=0.0, trans=False))
    cfg.Loss.update(dict(match=match, pc=0.2, a2fc=1.0, sw=5.0))
    net = vn.FACT(cfg, 16, V, N)
    net.mcriterion = MatchCriterion(cfg, A, [])
    gen = torch.Generator().manual_seed(seed)
    cuts = np.sort(rng.choice(np.arange(1, T), G - 1, replace=False))
    classes = rng.permutation(A)[:G] if match == "o2o" else rng.integers(0, A, G)
    label = torch.from_numpy(np.repeat(classes, np.diff(np.concatenate([[0], cuts, [T]])))).to(DEV)
    leaves = []

    def leaf(*shape):
        t = torch.randn(*shape, generator=gen).to(DEV).requires_grad_(True)
        leaves.append(t)
        return t
    for blk in net.block_list:
        tcuts = np.concatenate([[0], np.sort(rng.choice(np.arange(1, T), S - 1, replace=False)), [T]])
        st, en = torch.from_numpy(tcuts[:-1]).to(torch.int32), torch.from_numpy(tcuts[1:] - 1).to(torch.int32)
        sid = torch.from_numpy(np.repeat(np.arange(S), np.diff(tcuts))).to(torch.int32)
        tdu = TemporalDownsampleUpsample(sid.to(DEV), st.to(DEV), en.to(DEV))
        blk._save_logp(leaf(T, 1, V + N), leaf(S, 1, V + N), leaf(Q, 1, V + N + 2), tdu)
        if isinstance(blk, vn.UpdateBlockTDU):
            blk.f2a_attn_logit, blk.a2f_attn_logit = leaf(1, Q, S), leaf(1, S, Q)
            blk._save_attn(tdu, torch.softmax(blk.f2a_attn_logit.detach().transpose(2, 1), 1),
                           torch.softmax(blk.a2f_attn_logit.detach(), 2))
        else:
            blk._save_attn(None, None, None)
    m.tables(DEV), m.csr(DEV, V, N), m.csr(DEV, V + 1, N + 1)
    net.block_list[-1].a2f_attn      # (resolved: the per-term path's forward stores it)
    return dict(net=net, label=label, leaves=leaves)


def loss_phase(c, table):
    vn_vloss.FUSED_TABLE = table
    for t in c["leaves"]:
        t.grad = None
    lo = c["net"]._loss_one_video(c["label"])
    lo.backward()
    return lo


def timed(c, table, iters, warmup=3):
    for _ in range(warmup):
        loss_phase(c, table)
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        for t in c["leaves"]:
            t.grad = None
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        loss_phase(c, table)
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return round(statistics.median(ts), 1)


def peak(c, table):
    loss_phase(c, table)
    for t in c["leaves"]:
        t.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    lo = loss_phase(c, table)
    torch.cuda.synchronize()
    del lo
    return round((torch.cuda.max_memory_allocated() - base) / 1e6, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vn_table.json"))
    ap.add_argument("--commit", default=None, help="commit hash of the code under test, recorded in the output")
    args = ap.parse_args()
    shipped = vn_vloss.FUSED_TABLE
    res = {"commit": args.commit, "device": torch.cuda.get_device_name(0), "iters": args.iters,
           "unit": "median microseconds per loss phase (event-timed, host work included); peak MB above the inputs",
           "shapes": {}}
    for name, shp in SHAPES.items():
        c = make_case(**shp)
        lt = loss_phase(c, True)
        gt = [t.grad.clone() for t in c["leaves"]]
        lp = loss_phase(c, False)
        gp = [t.grad.clone() for t in c["leaves"]]
        out = dict(shp, cube_MB=round(shp["T"] * shp["Q"] * shp["G"] * 4 / 1e6, 2),
                   loss_table=float(lt.detach()), loss_per_term=float(lp.detach()),
                   grad_max_diff=max(float((a - b).abs().max()) for a, b in zip(gt, gp)),
                   table_peak_MB=peak(c, True), per_term_peak_MB=peak(c, False), table_us=[], per_term_us=[])
        for _ in range(args.rounds):                 # the two paths alternate
            out["table_us"].append(timed(c, True, args.iters))
            out["per_term_us"].append(timed(c, False, args.iters))
        out["table_slowest_beats_per_term_fastest"] = max(out["table_us"]) < min(out["per_term_us"])
        res["shapes"][name] = out
    vn_vloss.FUSED_TABLE = shipped
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
