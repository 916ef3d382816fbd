"""Whole-step time of the transcript-conditioned FACT on a batch whose transcripts have UNEQUAL lengths, with
``blocks.TRANS_RAGGED`` off -- one lockstep pass per video, each with its own term table, fx_loss_terms pair
and read-back -- and on: ONE pass with ragged token rows (fx_decoder_params.tok_off).

python tools/trans_ragged_time.py [--iters 10] [--rounds 3] [--out profiles/trans_ragged.json] [--commit HASH]

Model, widths, timing method and counters are tools/trans_step_time.py's (this imports them); the shape is four
videos of 1100-1900 frames with 24, 27, 30 and 33 transcript entries.  Both settings run the lockstep path
(TRANS_BATCH on); the comparison is against the switch-off path of the same tree.  Before timing both run once on
the timed inputs: losses, predictions and the largest gradient difference as a fraction of the tests' bound.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

import trans_step_time as ts  # noqa: E402
from factmx.models import blocks  # noqa: E402

VIDEOS = [(1500, 24, 1), (1100, 27, 2), (1900, 30, 3), (1300, 33, 4)]    # (frames, transcript entries, seed)


def step(c, ragged):
    blocks.TRANS_BATCH, blocks.TRANS_RAGGED = True, ragged
    net = c["net"]
    net.zero_grad(set_to_none=True)
    loss, saves = net(c["seqs"], c["labels"], compute_loss=True)
    loss.backward()
    return loss, saves


ts.step = step      # trans_step_time's timed / entry_calls / kernel_launches run this step


def compare(c):
    l0, s0 = step(c, False)
    s0 = [dict(s) for s in s0]
    g0 = {n: p.grad.clone() for n, p in c["net"].named_parameters()}
    l1, s1 = step(c, True)
    s1 = [dict(s) for s in s1]
    worst, who = 0.0, None    # as a fraction of the GPU tests' gradient bound rtol 2e-3 + 2e-3 RMS + 1e-6
    for n, p in c["net"].named_parameters():
        r = g0[n].double()
        tol = 2e-3 * r.abs() + 2e-3 * float(r.pow(2).mean().sqrt()) + 1e-6
        q = float(((p.grad.double() - r).abs() / tol).max())
        if q > worst:
            worst, who = q, n
    same = sum(int((a["pred"] == b["pred"]).sum()) for a, b in zip(s0, s1))
    total = sum(len(a["pred"]) for a in s0)
    rel = max(abs(a["loss"]["loss"] - b["loss"]["loss"]) / abs(a["loss"]["loss"]) for a, b in zip(s0, s1))
    return dict(loss_pass_per_video=float(l0.detach()), loss_one_pass=float(l1.detach()),
                per_video_loss_rel_diff=rel, equal_predictions=f"{same}/{total}",
                grad_diff_fraction_of_bound=worst, grad_diff_param=who, tdu_segments=c["net"].video_segments)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ts.ROOT, "profiles", "trans_ragged.json"))
    ap.add_argument("--commit", default=None, help="commit hash of the code under test, recorded in the output")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("trans_ragged_time: no GPU; a step time is only measured on the device")
    shipped = (blocks.TRANS_BATCH, blocks.TRANS_RAGGED)
    c = ts.make_case(VIDEOS)
    out = {"commit": args.commit, "device": torch.cuda.get_device_name(0), "iters": args.iters,
           "unit": "median milliseconds per step (zero_grad + forward + loss + backward; event-timed, host work "
                   "included); spread: range of the rounds' medians",
           "widths": "gtea_transcript.yaml: iuU, Bi sca hid 512 a_dim 128 a_layers 3 f_layers 10, Bu/BU sa, "
                     "D 2048, C 11, seq; dropout / cmr / TM off",
           "videos": VIDEOS}
    out.update(compare(c))
    out["ragged_off_ms"], out["ragged_on_ms"] = [], []
    for _ in range(args.rounds):                 # the two settings alternate
        out["ragged_off_ms"].append(ts.timed(c, False, args.iters))
        out["ragged_on_ms"].append(ts.timed(c, True, args.iters))
    for key in ("ragged_off_ms", "ragged_on_ms"):
        out[key + "_median"] = statistics.median(out[key])
        out[key + "_spread"] = round(max(out[key]) - min(out[key]), 3)
    out["ragged_off_fx_calls"], out["ragged_off_top_calls"] = ts.entry_calls(c, False)
    out["ragged_on_fx_calls"], out["ragged_on_top_calls"] = ts.entry_calls(c, True)
    out["ragged_off_kernels"] = ts.kernel_launches(c, False)
    out["ragged_on_kernels"] = ts.kernel_launches(c, True)
    blocks.TRANS_BATCH, blocks.TRANS_RAGGED = shipped
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
