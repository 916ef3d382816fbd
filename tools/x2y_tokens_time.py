"""Device time of one X2Y map (fx_x2y_fwd / fx_x2y_bwd through fxf.X2YFn) at more than 64 action tokens
per video: the wide fused cores of x2y_a2f.hip / x2y_f2a.hip against the grouped-GEMM path.

python tools/x2y_tokens_time.py [--iters 30] [--rounds 2] [--out FILE.json] [--commit HASH]
                                [--step-this BENCH.json] [--step-parent BENCH.json]

Shapes: both directions (a2f: keys = tokens, f2a: queries = tokens) at 75, 200 and 300 tokens, two
videos, at the frame shape (T = 4096 per video), at a segment shape (S = 100 per video; as KEYS, 100
segments are within the a2f cores' 320, so the f2a direction is also timed at S = 400, the f2a core's
segment-level class) and at the shipped yaml's segment count (S = 1700 per video; 75 tokens only),
H = 512, feature dims 256.  Each leg
runs in a CHILD process (the library reads its knobs once): "wide" with the defaults, "grouped" with
FX_X2Y_FUSED=0, which for these shapes is exactly what the code ran before the wide cores existed.  The
legs alternate (--rounds times each); a figure is the median over the rounds of the median of --iters
single event-timed calls after a warm-up, every call issued behind a filler GEMM so the host's launch
work is hidden.  "core" is fx_x2y_core's answer for the shape: at 0 the dispatch keeps the shape on the
grouped GEMMs and both legs time the same code; the wide f2a BACKWARD is opt-in (FX_X2Y_F2A_BWD=1), so
in the f2a rows of a default run only the forward differs between the legs.
--step-this / --step-parent: JSON lines of `bench.py --gpus 1 --config shipped` on this commit and on
its parent, whose ms_per_step are recorded beside the per-call times.  Prints one JSON object, and
writes it to --out.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fact-clip_amd"))

H, A, D2, OUT = 512, 256, 256, 256
NVID = 2
SHAPES = ([(d, lvl, n, tok) for d in ("a2f", "f2a") for lvl, n in (("frame", 4096), ("segment", 100))
           for tok in (75, 200, 300)] + [("f2a", "segment", 400, tok) for tok in (75, 200, 300)] +
          [(d, "segment_shipped", 1700, 75) for d in ("a2f", "f2a")])


def shape_name(d, lvl, n, tok):
    return f"{d}/{lvl}{n}/tok{tok}"


def leg(iters):
    """child: the times of every shape under this process's knobs"""
    import torch
    from factmx import functional as fxf
    dev = "cuda"
    fa, fb = torch.randn(2048, 2048, device=dev), torch.randn(2048, 2048, device=dev)

    def timed(fn, warmup=5):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.mm(fa, fb)      # filler: the device is busy while the host enqueues fn's launches
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        return round(statistics.median(ts), 2)

    res = {}
    for d, lvl, n, tok in SHAPES:
        g = torch.Generator().manual_seed(0)
        r = lambda *s: torch.randn(*s, generator=g).to(dev)   # noqa: E731
        nx, ny, xdim, ydim = (tok, n, A, D2) if d == "a2f" else (n, tok, D2, A)
        X, Y, Xp, Yp = r(NVID * nx, xdim), r(NVID * ny, ydim), r(NVID * nx, xdim), r(NVID * ny, ydim)
        rows = ([0, nx, 2 * nx], [0, ny, 2 * ny])
        W = [r(H, xdim) / xdim ** 0.5, r(H), r(H, xdim) / xdim ** 0.5, r(H), r(H, ydim) / ydim ** 0.5, r(H),
             r(OUT, ydim + H) / (ydim + H) ** 0.5, r(OUT)]

        def fwd():
            with torch.no_grad():
                fxf.X2YFn.apply(X, Y, Xp, Yp, rows, *W, 0.0, 0)
        leaves = [t.clone().requires_grad_(True) for t in (X, Y, Xp, Yp, *W)]
        out, logit, _ = fxf.X2YFn.apply(*leaves[:4], rows, *leaves[4:], 0.0, 0)
        gout, glog = r(*out.shape), r(*logit.shape)

        def bwd():
            torch.autograd.backward((out, logit), (gout, glog), retain_graph=True)
        res[shape_name(d, lvl, n, tok)] = {"fwd_us": timed(fwd), "bwd_us": timed(bwd)}
        fxf.check_device_status()
    print("LEG " + json.dumps(res), flush=True)


def run_leg(fused, iters):
    env = dict(os.environ)
    env.pop("FX_X2Y_FUSED", None)
    if not fused:
        env["FX_X2Y_FUSED"] = "0"
    p = subprocess.run([sys.executable, "-u", os.path.abspath(__file__), "--leg", "--iters", str(iters)], env=env,
                       cwd=ROOT, stdout=subprocess.PIPE, text=True, timeout=900)
    assert p.returncode == 0, p.returncode
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("LEG ")][-1][4:])


def step_ms(path):
    if not path:
        return None
    with open(path) as f:
        lines = [json.loads(ln) for ln in f if ln.lstrip().startswith("{")]
    return {"ms_per_step": lines[-1]["ms_per_step"], "steps": lines[-1]["steps"], "warmup": lines[-1]["warmup"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", action="store_true", help="(child) time every shape under this process's knobs")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="commit hash of the code under test, recorded in the output")
    ap.add_argument("--step-this", default=None)
    ap.add_argument("--step-parent", default=None)
    args = ap.parse_args()
    assert args.iters >= 20
    if args.leg:
        return leg(args.iters)
    from factmx import native as nx
    lib = nx.load()
    legs = {"wide": [], "grouped": []}
    for _ in range(args.rounds):
        legs["wide"].append(run_leg(True, args.iters))
        legs["grouped"].append(run_leg(False, args.iters))
    shapes = {}
    for d, lvl, n, tok in SHAPES:
        name = shape_name(d, lvl, n, tok)
        nxr, nyr = (tok, n) if d == "a2f" else (n, tok)
        core = lib.fx_x2y_core(H, NVID, nx.int_array([0, nxr, 2 * nxr]), nx.int_array([0, nyr, 2 * nyr]), 2 * nxr,
                               2 * nyr)
        e = {"core": core}
        for k in ("fwd_us", "bwd_us"):
            for lg in legs:
                e[f"{lg}_{k}"] = round(statistics.median(r[name][k] for r in legs[lg]), 2)
                e[f"{lg}_{k}_rounds"] = [r[name][k] for r in legs[lg]]
            e[f"speedup_{k[:3]}"] = round(e[f"grouped_{k}"] / e[f"wide_{k}"], 3)
        shapes[name] = e
    import torch
    res = {"commit": args.commit, "device": torch.cuda.get_device_name(0), "videos": NVID, "iters": args.iters,
           "rounds": args.rounds, "shapes": shapes,
           "bench_shipped": {"this": step_ms(args.step_this), "parent": step_ms(args.step_parent)}}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
