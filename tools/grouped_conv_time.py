"""Device time of the dilated Conv1d(k=3) layer, dense and grouped, and of one training step.

python tools/grouped_conv_time.py [--dense-only] [--iters 25] [--out FILE.json] [--commit HASH]

Times fxf.conv3 at rows = 2 x 4096, F = 512, dilation 16 with HIP events: the forward, the input
gradient alone (only x requires grad) and the weight + bias gradient alone (only w, b require grad);
each figure is the median of --iters single calls after a warm-up, every call issued behind a filler
GEMM so the host's launch work is hidden and the event pair brackets device work only.  Without
--dense-only it times the grouped layer (g = 4) too, and one forward + backward step of the benchmark's
FACT_CLIP with Bi.f_dim = 512, f_ln = True for Bi.f_ngp = 4 and 1.  --dense-only uses nothing beyond
the dense fxf.conv3, so it also runs on a checkout that predates the grouped kernels (the baseline
leg).  Prints one JSON object, and writes it to --out.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fact-clip_amd"))

import torch  # noqa: E402

from factmx import functional as fxf  # noqa: E402

DEV = "cuda"


class Timer:
    def __init__(self, iters):
        self.iters = iters
        self.fa = torch.randn(2048, 2048, device=DEV)
        self.fb = torch.randn(2048, 2048, device=DEV)

    def __call__(self, fn, warmup=5):
        """median / min / max microseconds of fn() over iters single event-timed calls"""
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(self.iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.mm(self.fa, self.fb)      # filler: the device is busy while the host enqueues fn's launches
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        return dict(median_us=round(statistics.median(ts), 2), min_us=round(min(ts), 2), max_us=round(max(ts), 2),
                    n=len(ts))


def conv_times(timer, F, g, T, nvid, dil):
    rows = T * nvid
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(rows, F, generator=gen).to(DEV)
    w = (torch.randn(F, F // g, 3, generator=gen) / (3 * F // g) ** 0.5).to(DEV)
    b = torch.randn(F, generator=gen).to(DEV)
    gy = torch.randn(rows, F, generator=gen).to(DEV)
    out = {"F": F, "g": g, "rows": rows, "T": T, "dil": dil, "flops": 2.0 * rows * F * 3 * (F // g)}

    def fwd():
        with torch.no_grad():
            fxf.conv3(x, w, b, dil, T)
    out["fwd"] = timer(fwd)

    def make(xg, wg):
        xs, ws, bs = x.clone().requires_grad_(xg), w.clone().requires_grad_(wg), b.clone().requires_grad_(wg)
        y = fxf.conv3(xs, ws, bs, dil, T)
        return lambda: y.backward(gy, retain_graph=True)
    out["dx"] = timer(make(True, False))
    out["dw"] = timer(make(False, True))
    return out


def step_times(timer, ngp):
    import bench
    cfg = bench.make_cfg()
    cfg.Bi.f_dim, cfg.Bi.f_ngp, cfg.Bi.f_ln = 512, ngp, True
    T, D, C, nv = 4096, 2048, bench.NCLS, 2
    net, _ = bench.build_model(cfg, D, C, device=DEV, seed=0)
    net.train()
    vids = [bench.make_video(T, D, C, cfg, seed=100 + v) for v in range(nv)]
    seqs = [torch.from_numpy(f).float().to(DEV) for f, _ in vids]
    labs = [torch.from_numpy(l).to(DEV) for _, l in vids]

    def step():
        net.zero_grad(set_to_none=False)
        loss, _ = net(seqs, labs, compute_loss=True)
        loss.backward()
    r = timer(step, warmup=3)
    fxf.check_device_status()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dense-only", action="store_true")
    ap.add_argument("--iters", type=int, default=25)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="commit hash of the code under test, recorded in the output")
    args = ap.parse_args()
    assert args.iters >= 20
    timer = Timer(args.iters)
    res = {"commit": args.commit, "device": torch.cuda.get_device_name(0),
           "dense": conv_times(timer, 512, 1, 4096, 2, 16)}
    if not args.dense_only:
        res["grouped"] = conv_times(timer, 512, 4, 4096, 2, 16)
        res["step_f_ngp4"] = step_times(Timer(20), 4)
        res["step_f_ngp1"] = step_times(Timer(20), 1)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
