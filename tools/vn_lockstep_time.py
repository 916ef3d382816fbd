"""Whole-step time of the verb/noun FACT (models/blocks_SepVerbNoun.py) with ``LOCKSTEP`` off -- the videos
one by one, one loss table per video -- and on: every block over the stacked videos, one matching-cost
launch, one loss table, one prediction pass and one read-back per step (models/vn_vloss.run_batch).

python tools/vn_lockstep_time.py [--iters 10] [--rounds 3] [--shapes tiny_vn_batch,epic_like]
                                 [--out profiles/vn_lockstep.json] [--commit HASH]

Two shapes: the ``tiny_vn_batch`` fixture's (3 videos of 150 / 97 / 211 frames, 5 / 7 heads, 12 actions, 8
tokens, IUU, o2o) and an EPIC-like one (4 videos of about 4096 frames, ragged; 98 / 301 heads, 4000 actions,
300 tokens, IUUU, o2m, the widths of the reference's epic-kitchens configuration; synthetic segmented
inputs, 130 ground-truth segments per video; torch's own seeded initialisation -- with the fixtures'
paramgen weights at these widths the last block's segmentation collapses to one segment per video).  A step is zero_grad + forward + loss + backward on the same
model and inputs for both paths.  HIP events around single steps after a warm-up (host work -- the
segment-count reads, the matching, launches -- is inside the interval, and each step ends in a device
synchronise); each figure is the median of --iters steps, the two paths alternate --rounds times, and the
spread is the range of the rounds' medians.  Before timing, both paths run once on the same inputs and
their losses, predictions and gradients are compared.  Launches per step: calls of the library's fx_*
entries (counted by wrapping the binding) and, where the profiler is available, device kernels of one
step from torch.profiler, in a pass of its own.  Prints one JSON object and writes it to --out.
"""
import argparse
import collections
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fact-clip_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import paramgen as pg  # noqa: E402
from factmx import native as nx  # noqa: E402
from factmx.configs import get_cfg_defaults  # noqa: E402
from factmx.models import blocks_SepVerbNoun as vn  # noqa: E402
from factmx.models.loss import MatchCriterion  # noqa: E402

DEV = "cuda"
SHAPES = {
    "tiny_vn_batch": dict(videos=[(150, 4, 1), (97, 3, 3), (211, 5, 2)], D=40, V=5, N=7, A=12, Q=8, block="IUU",
                          match="o2o", nullw=1.0 / 6,
                          Bi=dict(hid_dim=48, a="sca", a_nhead=4, a_ffdim=48, a_layers=2, a_dim=32, f="m", f_layers=3,
                                  f_dim=24),
                          BU=dict(f_layers=3, a_nhead=4, s_layers=1)),
    "epic_like": dict(videos=[(4096, 130, 1), (3584, 130, 2), (4352, 130, 3), (3968, 130, 4)], D=512, V=98, N=301,
                      A=4000, Q=300, block="IUUU", match="o2m", nullw=0.05, init="torch",
                      Bi=dict(hid_dim=512, a="sca", a_nhead=8, a_ffdim=512, a_layers=6, a_dim=256, f="m2", f_layers=10,
                              f_dim=256),
                      BU=dict(a="sa", a_layers=1, a_nhead=8, f_layers=10, s_layers=1)),
}


def make_case(videos, D, V, N, A, Q, block, match, nullw, Bi, BU, init="paramgen", seed=0):
    rng = np.random.default_rng(seed)
    if A == 12:
        vids, nids = [0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 0, 2], [0, 1, 2, 3, 4, 5, 6, 0, 1, 2, 3, 6]
    else:
        vids, nids = rng.integers(0, V, A), rng.integers(0, N, A)
        vids[-1], nids[-1] = V - 1, N - 1
        vids, nids = vids.tolist(), nids.tolist()
    m = vn.set_verb_noun_ids(vids, nids)
    cfg = get_cfg_defaults()
    cfg.Bi.update(dict(Bi, dropout=0.0, f_ln=False, f_ngp=1))
    cfg.BU.update(BU)
    cfg.FACT.update(dict(ntoken=Q, block=block, cmr=0.0, fpos=True, trans=False))
    cfg.Loss.update(dict(match=match, pc=0.2, a2fc=1.0, sw=5.0, nullw=nullw))
    cfg.TM.use = False
    torch.manual_seed(seed)
    net = vn.FACT(cfg, D, V, N)
    if init == "paramgen":          # the fixtures' weights; otherwise torch's own initialisation under the seed
        with torch.no_grad():
            for n, p in net.named_parameters():
                p.copy_(torch.from_numpy(pg.param_value(n, p.shape, 1)))
    net.mcriterion = MatchCriterion(cfg, A, [])
    net = net.to(DEV).train()
    seqs, labels = [], []
    for T, nseg, s in videos:
        classes = list(range(A)) if match == "o2o" else rng.integers(0, A, 40).tolist()
        f, l_ = pg.segmented_video(T, D, classes, nseg, seed=s, noise=0.3)
        seqs.append(torch.from_numpy(f).float().to(DEV))
        labels.append(torch.from_numpy(l_).to(DEV))
    m.tables(DEV), m.csr(DEV, V, N), m.csr(DEV, V + 1, N + 1)
    return dict(net=net, seqs=seqs, labels=labels)


def step(c, lockstep):
    vn.LOCKSTEP = lockstep
    net = c["net"]
    net.zero_grad(set_to_none=True)
    loss, saves = net(c["seqs"], c["labels"], compute_loss=True)
    loss.backward()
    return loss, saves


def timed(c, lockstep, iters, warmup=3):
    for _ in range(warmup):
        step(c, lockstep)
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        step(c, lockstep)
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return round(statistics.median(ts), 3)


def entry_calls(c, lockstep):
    """fx_* entry calls of one step, by wrapping the binding's functions."""
    lib = nx.load()
    counts = collections.Counter()
    orig = {}
    skip = ("fx_last_error", "fx_version", "fx_struct_size", "fx_side_stream", "fx_get_stream_precision",
            "fx_stream_precision_explicit", "fx_get_default_precision")
    for name in nx.SIGNATURES:
        if name in skip or name.endswith("_floats"):
            continue
        fn = getattr(lib, name)
        orig[name] = fn

        def wrapped(*a, _fn=fn, _n=name):
            counts[_n] += 1
            return _fn(*a)
        setattr(lib, name, wrapped)
    try:
        step(c, lockstep)
        torch.cuda.synchronize()
    finally:
        for name, fn in orig.items():
            setattr(lib, name, fn)
    return sum(counts.values()), dict(counts.most_common(8))


def kernel_launches(c, lockstep):
    """Device kernels of one step (torch.profiler); None where the profiler gives no device events."""
    try:
        from torch.profiler import profile, ProfilerActivity
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            step(c, lockstep)
            torch.cuda.synchronize()
        n = sum(1 for ev in prof.events() if str(ev.device_type).endswith("CUDA") and "emcpy" not in ev.name
                and "emset" not in ev.name)
        return n or None
    except Exception as e:      # noqa: BLE001  (a profiler that cannot trace here: not measured)
        print("kernel count not measured:", e, file=sys.stderr)
        return None


def compare(c):
    """Both paths once on the same inputs: losses, predictions, the largest gradient difference as a
    fraction of the tests' bound."""
    l0, s0 = step(c, False)
    g0 = {n: p.grad.clone() for n, p in c["net"].named_parameters()}
    l1, s1 = step(c, True)
    segs1 = c["net"].video_segments
    worst = 0.0            # as a fraction of the GPU tests' gradient bound rtol 2e-3 + 2e-3 RMS + 1e-6
    for n, p in c["net"].named_parameters():
        r = g0[n].double()
        tol = 2e-3 * r.abs() + 2e-3 * float(r.pow(2).mean().sqrt()) + 1e-6
        worst = max(worst, float(((p.grad.double() - r).abs() / tol).max()))
    same = sum(int((a["pred"] == b["pred"]).sum()) for a, b in zip(s0, s1))
    total = sum(len(a["pred"]) for a in s0)
    return dict(loss_per_video_path=float(l0.detach()), loss_lockstep=float(l1.detach()),
                equal_predictions=f"{same}/{total}", grad_diff_fraction_of_bound=worst, tdu_segments=segs1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vn_lockstep.json"))
    ap.add_argument("--commit", default=None, help="commit hash of the code under test, recorded in the output")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vn_lockstep_time: no GPU; a step time is only measured on the device")
    shipped = vn.LOCKSTEP
    res = {"commit": args.commit, "device": torch.cuda.get_device_name(0), "iters": args.iters,
           "unit": "median milliseconds per step (zero_grad + forward + loss + backward; event-timed, host work "
                   "included); spread: range of the rounds' medians",
           "shapes": {}}
    for name in args.shapes.split(","):
        shp = SHAPES[name]
        c = make_case(**shp)
        out = dict(videos=shp["videos"], heads=[shp["V"], shp["N"]], actions=shp["A"], tokens=shp["Q"],
                   block=shp["block"], match=shp["match"], init=shp.get("init", "paramgen"))
        out.update(compare(c))
        out["per_video_ms"], out["lockstep_ms"] = [], []
        for _ in range(args.rounds):                 # the two paths alternate
            out["per_video_ms"].append(timed(c, False, args.iters))
            out["lockstep_ms"].append(timed(c, True, args.iters))
        for key in ("per_video_ms", "lockstep_ms"):
            out[key + "_median"] = statistics.median(out[key])
            out[key + "_spread"] = round(max(out[key]) - min(out[key]), 3)
        out["per_video_fx_calls"], out["per_video_top_calls"] = entry_calls(c, False)
        out["lockstep_fx_calls"], out["lockstep_top_calls"] = entry_calls(c, True)
        out["per_video_kernels"] = kernel_launches(c, False)
        out["lockstep_kernels"] = kernel_launches(c, True)
        res["shapes"][name] = out
        print(name, json.dumps(out), flush=True)
        if args.out:                                 # (written after every shape: a later shape may run long)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
    vn.LOCKSTEP = shipped
    print(json.dumps(res))


if __name__ == "__main__":
    main()
