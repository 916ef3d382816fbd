"""Diagnostic: a 10-layer F = 256 MS-TCN++ stack (in_map off) on 2 x 4096 rows, the fused layer kernel
(functional.MSTCN2_FUSED_LAYERS = 2) against the GEMM launches of the same build (= 0).  Forward alone and
forward + backward are timed with HIP events after a warm-up; the two paths alternate in rounds, and the
report gives the median of each and the range of the rounds' medians.  The fused chains' own time per launch
comes from the fx_prof brackets (native.PROF_MSTCN2_FUSED) of one extra step.  --epic-step adds the verb/noun
model's whole step at the `epic_like` shape with the knob at 0 and at 1, --fill-sweep both paths on fewer rows
(where the fused path breaks even: FX_FRL2_MIN_FILL).  Writes profiles/m2_fused_layer.json
(python tools/m2_layer_bench.py [--rounds 3] [--steps 20] [--epic-step] [--fill-sweep] [--out PATH])."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fact-clip_amd"))

import torch  # noqa: E402

from factmx import functional as fxf  # noqa: E402
from factmx import native as nx  # noqa: E402
from factmx.dp import FlatGradReducer  # noqa: E402
from factmx.models.basic import MSTCN2  # noqa: E402

F, NL, T, NVID = 256, 10, 4096, 2
PEAK_F32_TFLOPS = 157.3
PATHS = {"gemm": 0, "fused": 2}


def _timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps * 1e3      # us per call


def _chain_us(lib, fn):
    """us per launch of the fused chains fn() brackets (0 launches: None)."""
    nx.check(lib.fx_prof_enable(nx.PROF_MSTCN2_FUSED, 64), "fx_prof_enable")
    try:
        fn()
        torch.cuda.synchronize()
        ms, fl, by, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
        nx.check(lib.fx_prof_collect(nx.PROF_MSTCN2_FUSED, ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by),
                                     ctypes.byref(n)), "fx_prof_collect")
    finally:
        lib.fx_prof_disable()
    return (ms.value * 1e3 / n.value, n.value) if n.value else (None, 0)


def epic_step(rounds, iters=10):
    """The verb/noun model's whole lockstep step at tools/vn_lockstep_time.py's `epic_like` shape (16,000 frame
    rows through four 10-layer F = 256 'm2' stacks), MSTCN2_FUSED_LAYERS 0 against 1 (the default rule: the
    fill threshold applies), alternated in one process: median ms per step and the range of the rounds."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import vn_lockstep_time as vt
    c = vt.make_case(**vt.SHAPES["epic_like"])
    out = {"unit": "median ms per epic_like lockstep step (zero_grad + forward + loss + backward)", "iters": iters}
    ms = {0: [], 1: []}
    for knob in ms:
        fxf.MSTCN2_FUSED_LAYERS = knob
        out[f"loss_knob{knob}"] = float(vt.step(c, True)[0].detach())
    for _ in range(rounds):
        for knob in ms:
            fxf.MSTCN2_FUSED_LAYERS = knob
            ms[knob].append(vt.timed(c, True, iters))
    for knob, v in ms.items():
        out[f"knob{knob}_ms"] = {"median": statistics.median(v), "rounds": v, "range": round(max(v) - min(v), 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--epic-step", action="store_true", help="also time the epic_like whole step, knob 0 against 1")
    ap.add_argument("--fill-sweep", action="store_true", help="also time both paths at 25-80 %% of one row tile per CU")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "m2_fused_layer.json"))
    args = ap.parse_args()
    assert args.rounds >= 3
    lib = nx.load()
    torch.manual_seed(0)
    mod = MSTCN2(F, F, F, NL, dropout=0.0, in_map=False).cuda().train()
    FlatGradReducer(mod.parameters())     # uniformly strided gradients: the batched weight-gradient launches
    rows = T * NVID
    x = torch.randn(rows, F, device="cuda", requires_grad=True)
    g = torch.randn(rows, F, device="cuda")

    def fwd():
        with torch.no_grad():
            return fxf.mstcn2(mod, x, T, NVID)

    def fwd_bwd():
        fxf.mstcn2(mod, x, T, NVID).backward(g)

    # the two paths compute the same thing
    outs = {}
    for name, knob in PATHS.items():
        fxf.MSTCN2_FUSED_LAYERS = knob
        x.grad = None
        y = fxf.mstcn2(mod, x, T, NVID)
        y.backward(g)
        outs[name] = (y.detach().clone(), x.grad.detach().clone())
    # (max: a ReLU gate within fp32 rounding of 0 may fall on either side in the two paths and moves single
    # gradient entries; rms: the difference over all entries)
    def rel(a, b, how):
        return (how((a - b).double()) / how(b.double())).item()
    dmax = {k: rel(outs["fused"][i], outs["gemm"][i], lambda t: t.abs().max()) for i, k in enumerate(("y", "dx"))}
    drms = {k: rel(outs["fused"][i], outs["gemm"][i], lambda t: t.pow(2).mean().sqrt()) for i, k in enumerate(("y", "dx"))}

    med = {n: {"fwd": [], "fwd_bwd": []} for n in PATHS}
    for _ in range(args.rounds):
        for name, knob in PATHS.items():
            fxf.MSTCN2_FUSED_LAYERS = knob
            for what, fn in (("fwd", fwd), ("fwd_bwd", fwd_bwd)):
                for _w in range(args.warmup):
                    fn()
                med[name][what].append(statistics.median(_timed(fn, args.steps) for _s in range(5)))
    fxf.MSTCN2_FUSED_LAYERS = 2
    f_us, f_n = _chain_us(lib, fwd)

    def bwd_only_chain():
        y = fxf.mstcn2(mod, x, T, NVID)
        nx.check(lib.fx_prof_enable(nx.PROF_MSTCN2_FUSED, 64), "fx_prof_enable")   # (drop the forward's bracket)
        y.backward(g)
    b_us, b_n = _chain_us(lib, bwd_only_chain)
    flop = 2.0 * rows * F * 8 * F           # per forward launch: two K = 3F convs and the K = 2F fusion
    res = {
        "shape": {"F": F, "layers": NL, "rows": rows, "T": T, "videos": NVID, "in_map": False},
        "device": torch.cuda.get_device_name(0),
        "rounds": args.rounds, "steps_per_sample": args.steps, "samples_per_round": 5,
        "fill_threshold_pct": int(os.environ.get("FX_FRL2_MIN_FILL", 55)),
        "row_tiles": (rows + 31) // 32,
        "rel_diff_fused_vs_gemm": {"max": dmax, "rms": drms},
        "fused_chain": {"fwd_us_per_launch": f_us, "fwd_launches": f_n, "bwd_us_per_launch": b_us, "bwd_launches": b_n,
                        "fwd_frac_f32_peak": (flop / (f_us * 1e-6) / 1e12 / PEAK_F32_TFLOPS) if f_us else None},
    }
    for name in PATHS:
        for what in ("fwd", "fwd_bwd"):
            v = med[name][what]
            res[f"{name}_{what}_us"] = {"median": statistics.median(v), "round_medians": v, "range": max(v) - min(v)}
    for what in ("fwd", "fwd_bwd"):
        gm, fm = res[f"gemm_{what}_us"], res[f"fused_{what}_us"]
        res[f"{what}_fused_faster_beyond_range"] = gm["median"] - fm["median"] > max(gm["range"], fm["range"])
    res["gemm_fwd_us_per_layer"] = res["gemm_fwd_us"]["median"] / NL
    if args.fill_sweep:
        # where the fused path breaks even: the same stack on fewer rows (2 videos), fill = row tiles / CUs
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        res["fill_sweep"] = []
        for pct in (25, 40, 50, 55, 60, 65, 80):
            t_ = max(cus * pct // 100 // 2, 1) * 32            # rows per video
            xs = torch.randn(2 * t_, F, device="cuda", requires_grad=True)
            gs = torch.randn(2 * t_, F, device="cuda")
            row = {"fill_pct": pct, "rows": 2 * t_, "row_tiles": 2 * t_ // 32}
            ms = {n: {"fwd": [], "fwd_bwd": []} for n in PATHS}
            for _ in range(args.rounds):
                for name, knob in PATHS.items():
                    fxf.MSTCN2_FUSED_LAYERS = knob

                    def f1():
                        with torch.no_grad():
                            fxf.mstcn2(mod, xs, t_, 2)

                    def f2():
                        fxf.mstcn2(mod, xs, t_, 2).backward(gs)
                    for what, fn in (("fwd", f1), ("fwd_bwd", f2)):
                        for _w in range(args.warmup):
                            fn()
                        ms[name][what].append(statistics.median(_timed(fn, args.steps) for _s in range(3)))
            for name in PATHS:
                for what in ("fwd", "fwd_bwd"):
                    v = ms[name][what]
                    row[f"{name}_{what}_us"] = {"median": statistics.median(v), "range": max(v) - min(v)}
            res["fill_sweep"].append(row)
    if args.epic_step:
        res["epic_like_step"] = epic_step(args.rounds)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fp:
        json.dump(res, fp, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
