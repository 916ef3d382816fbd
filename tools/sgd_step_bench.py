"""FusedSGD.step() (momentum 0.9, clip on) against clip_grad_norm_ + torch.optim.SGD(foreach).step() on the
parameter set of bench.py's default model.

Both sides get the same gradients, restored before every timed step (outside the timed window) so that the
clip rewrites the gradient every time: the fused step then moves 24 B per parameter (+4 B for the norm's
read of g).  Fused and eager steps alternate in one process; every step is timed by its own pair of device
events.  Prints one line per side and one JSON line.

  python tools/sgd_step_bench.py [--reps 200] [--warmup 20]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "fact-clip_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK = 8.0e12        # B/s, the MI355X HBM3E specification peak
MAX_NORM, LR, MOMENTUM = 10.0, 0.1, 0.9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    import torch
    import bench
    from factmx.optim import FusedSGD
    if not torch.cuda.is_available():
        sys.exit("sgd_step_bench: needs the GPU (no timing without one)")
    dev = "cuda"
    cfg, D, C, _, _, clip, _ = bench.workload("default")
    net, _ = bench.build_model(cfg, D, C, dev, clip=clip)
    mine = [p for p in net.parameters() if p.requires_grad]
    ref = [torch.nn.Parameter(p.detach().clone()) for p in mine]
    n = sum(p.numel() for p in mine)
    opt = FusedSGD(mine, lr=LR, momentum=MOMENTUM, max_grad_norm=MAX_NORM)
    opt_ref = torch.optim.SGD(ref, lr=LR, momentum=MOMENTUM, foreach=True)
    gen = torch.Generator(device=dev).manual_seed(0)
    g0 = torch.randn(n, device=dev, generator=gen) * 0.01      # ||g|| = 0.01 sqrt(n) ~ 54 > max_norm: coef < 1
    for p in ref:
        p.grad = torch.empty_like(p)
    ref_grads = [p.grad for p in ref]
    g0_views, off = [], 0
    for p in ref:
        g0_views.append(g0[off:off + p.numel()].view_as(p))
        off += p.numel()

    def fused():
        opt.grad_flat.copy_(g0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        opt.step()
        e1.record()
        return e0, e1

    def eager():
        torch._foreach_copy_(ref_grads, g0_views)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.nn.utils.clip_grad_norm_(ref, MAX_NORM)
        opt_ref.step()
        e1.record()
        return e0, e1

    for _ in range(args.warmup):
        fused()
        eager()
    torch.cuda.synchronize()
    assert opt.total_norm.item() > MAX_NORM, "the clip must be active in the timed steps"
    ev = {"fused": [], "eager": []}
    for _ in range(args.reps):
        ev["fused"].append(fused())
        ev["eager"].append(eager())
    torch.cuda.synchronize()
    out = {"params": n, "tensors": len(mine), "reps": args.reps, "warmup": args.warmup,
           "bytes_per_param": 24, "hbm_peak_Bps": HBM_PEAK}
    for name, pairs in ev.items():
        us = sorted(1e3 * a.elapsed_time(b) for a, b in pairs)
        q = statistics.quantiles(us, n=20)
        out[name] = dict(median_us=round(statistics.median(us), 2), p5_us=round(q[0], 2), p95_us=round(q[-1], 2),
                         min_us=round(us[0], 2), max_us=round(us[-1], 2))
        print(f"{name}: median {out[name]['median_us']} us  p5 {out[name]['p5_us']}  p95 {out[name]['p95_us']}  "
              f"min {out[name]['min_us']}  max {out[name]['max_us']}  ({args.reps} steps)")
    bps = 24.0 * n / (out["fused"]["median_us"] * 1e-6)
    out["fused_Bps"] = round(bps, -9)
    out["fused_frac_of_hbm_peak"] = round(bps / HBM_PEAK, 3)
    out["eager_over_fused"] = round(out["eager"]["median_us"] / out["fused"]["median_us"], 2)
    err = (opt.flat - torch.cat([p.detach().reshape(-1) for p in ref])).abs().max().item()
    out["max_param_diff_fused_vs_eager"] = err      # both ran warmup + reps steps on the same gradients
    print(json.dumps(out))


if __name__ == "__main__":
    main()
