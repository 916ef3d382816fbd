"""Whole-step time of the transcript-conditioned FACT (``FACT.trans``, models/blocks.py) with
``blocks.TRANS_BATCH`` off -- every video alone through the blocks, the per-video loss methods and the eager
transcript prediction -- and on: the lockstep pass on the embedded transcript tokens, one term table, one
fx_loss_terms pair, fx_eval_pred_trans and one read-back per pass.

python tools/trans_step_time.py [--iters 10] [--rounds 3] [--shapes batch1,batch4]
                                [--out profiles/trans_lockstep.json] [--commit HASH]

The widths are gtea_transcript.yaml's (block iuU, Bi: sca, hid 512, a_dim 128, 3 decoder layers, 10 frame
layers; Bu / BU: sa, 3 / 5 frame layers; D = 2048, C = 11, seq matching, sw 5) with dropout, channel masking
and time masking off, so that both paths compute the same function and can be compared.  Synthetic segmented
videos of 1100-1900 frames with 30 transcript entries each: one video (the shipped batch size), and a batch of
four with equal transcript lengths (one pass).  A step is zero_grad + forward + loss + backward on the same
model and inputs for both paths; HIP events around single steps after a warm-up (host work is inside the
interval, each step ends in a device synchronise); each figure is the median of --iters steps, the two paths
alternate --rounds times, and the spread is the range of the rounds' medians.  Before timing both paths run
once and their losses, predictions and gradients are compared.  Launches per step: calls of the library's
fx_* entries (counted by wrapping the binding) and, where the profiler is available, device kernels of one
step from torch.profiler.  Prints one JSON object and writes it to --out.
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

import torch  # noqa: E402

import paramgen as pg  # noqa: E402
from factmx import native as nx  # noqa: E402
from factmx.configs import get_cfg_defaults  # noqa: E402
from factmx.models import blocks  # noqa: E402
from factmx.models.loss import MatchCriterion  # noqa: E402

DEV = "cuda"
D, C = 2048, 11
SHAPES = {      # (frames, transcript entries, video seed)
    "batch1": [(1500, 30, 1)],
    "batch4": [(1500, 30, 1), (1100, 30, 2), (1900, 30, 3), (1300, 30, 4)],
}


def make_case(videos, seed=0):
    cfg = get_cfg_defaults()
    cfg.Bi.update(dict(hid_dim=512, dropout=0.0, a="sca", a_nhead=8, a_ffdim=512, a_layers=3, a_dim=128, f="m",
                       f_layers=10, f_ln=False, f_dim=128, f_ngp=1))
    cfg.Bu.update(dict(a="sa", a_layers=1, a_nhead=8, f_layers=3))
    cfg.BU.update(dict(a="sa", a_layers=1, a_nhead=8, f_layers=5, s_layers=1))
    cfg.FACT.update(dict(ntoken=0, block="iuU", cmr=0.0, fpos=False, mwt=0.0, trans=True))
    cfg.Loss.update(dict(match="seq", pc=1.0, a2fc=1.0, sw=5.0, bgw=1.0, nullw=1.0))
    cfg.TM.use = False
    torch.manual_seed(seed)
    net = blocks.FACT(cfg, D, C)
    net.mcriterion = MatchCriterion(cfg, C, [])
    net = net.to(DEV).train()
    seqs, labels = [], []
    for T, nseg, s in videos:
        f, l_ = pg.segmented_video(T, D, list(range(C)), nseg, seed=s, noise=0.3)
        seqs.append(torch.from_numpy(f).float().to(DEV))
        labels.append(torch.from_numpy(l_).to(DEV))
    return dict(net=net, seqs=seqs, labels=labels)


def step(c, batch):
    blocks.TRANS_BATCH = batch
    net = c["net"]
    net.zero_grad(set_to_none=True)
    loss, saves = net(c["seqs"], c["labels"], compute_loss=True)
    loss.backward()
    return loss, saves


def timed(c, batch, iters, warmup=3):
    for _ in range(warmup):
        step(c, batch)
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        step(c, batch)
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return round(statistics.median(ts), 3)


def entry_calls(c, batch):
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
        step(c, batch)
        torch.cuda.synchronize()
    finally:
        for name, fn in orig.items():
            setattr(lib, name, fn)
    return sum(counts.values()), dict(counts.most_common(8))


def kernel_launches(c, batch):
    """Device kernels of one step (torch.profiler); None where the profiler gives no device events."""
    try:
        from torch.profiler import profile, ProfilerActivity
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            step(c, batch)
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
    s0 = [dict(s) for s in s0]
    g0 = {n: p.grad.clone() for n, p in c["net"].named_parameters()}
    l1, s1 = step(c, True)
    worst = 0.0            # as a fraction of the GPU tests' gradient bound rtol 2e-3 + 2e-3 RMS + 1e-6
    for n, p in c["net"].named_parameters():
        r = g0[n].double()
        tol = 2e-3 * r.abs() + 2e-3 * float(r.pow(2).mean().sqrt()) + 1e-6
        worst = max(worst, float(((p.grad.double() - r).abs() / tol).max()))
    same = sum(int((a["pred"] == b["pred"]).sum()) for a, b in zip(s0, s1))
    total = sum(len(a["pred"]) for a in s0)
    return dict(loss_per_video_path=float(l0.detach()), loss_lockstep=float(l1.detach()),
                equal_predictions=f"{same}/{total}", grad_diff_fraction_of_bound=worst,
                tdu_segments=c["net"].video_segments)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trans_lockstep.json"))
    ap.add_argument("--commit", default=None, help="commit hash of the code under test, recorded in the output")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("trans_step_time: no GPU; a step time is only measured on the device")
    shipped = blocks.TRANS_BATCH
    res = {"commit": args.commit, "device": torch.cuda.get_device_name(0), "iters": args.iters,
           "unit": "median milliseconds per step (zero_grad + forward + loss + backward; event-timed, host work "
                   "included); spread: range of the rounds' medians",
           "widths": "gtea_transcript.yaml: iuU, Bi sca hid 512 a_dim 128 a_layers 3 f_layers 10, Bu/BU sa, "
                     "D 2048, C 11, seq; dropout / cmr / TM off",
           "shapes": {}}
    for name in args.shapes.split(","):
        c = make_case(SHAPES[name])
        out = dict(videos=SHAPES[name])
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
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
    blocks.TRANS_BATCH = shipped
    print(json.dumps(res))


if __name__ == "__main__":
    main()
