"""The tile orders of fx_gemm (block_tile / block_tile_id in csrc/gemm_dev.h: xcd_planes, row_perm, group_m, and the
wide kernel's persistent grid) and the 64 x 64 kernel's in-launch split-K reduction, one launch per case, at
shapes where a wrong mapping shows: a last group with fewer row tiles than group_m, a tile count that is no
multiple of the persistent grid, plane counts on both sides of "a multiple of 8", a ragged last row tile (GPU).

A remap that is not a bijection computes one tile twice and leaves another unwritten, so every output (and every
split-K workspace) starts as NaN and EVERY element is compared with float64 torch on the same fp32 inputs, at
the tolerance of tests/test_gpu_gemm.py; the count of NaN or out-of-tolerance elements must be 0, and a failure
prints the (ty, tx) tiles that hold them.  Each case first asserts, through fx_gemm_plan on the very descriptor
it launches, the plan it stands on (tests/gemm_cases.py), so a moved threshold fails there instead of silently
testing another path.

A remap changes which workgroup computes a tile, never an operation or the k order, so a child process with
the four knobs off must produce the same bits.  Library knobs are read once per process."""
import functools
import os
import subprocess
import sys

import pytest
import torch

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (_ROOT, os.path.join(_ROOT, "fact-clip_amd"), os.path.join(_ROOT, "tests")):   # (the child has no conftest)
    if _p not in sys.path:
        sys.path.insert(0, _p)

import gemm_cases as gc  # noqa: E402
from factmx import native as nx  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = {c[0]: c for c in gc.TILE_CASES}

# run id -> (case id, variant, plan fields that differ from the case's).  Variants: plain; beta_gate (the epilogue
# of test_gemm: beta 0.5 on a known C, gated); bf16 / fp32s (the stream's precision: gemm_bf16.hip's and, with B
# column-major, gemm_split.hip's block_tile); ones_col (B's virtual ones column into c_last, beta 1).
RUNS = {c[0]: (c[0], "plain", {}) for c in gc.TILE_CASES}
RUNS.update({
    "row_perm_2-bf16": ("row_perm_2", "bf16", dict(family=gc.BF16)),
    "row_perm_3-bf16": ("row_perm_3", "bf16", dict(family=gc.BF16)),
    "row_perm_off_17-bf16": ("row_perm_off_17", "bf16", dict(family=gc.BF16)),
    # the grouped order with a partial last group on the split kernel (no persistent grid there)
    "persist_group_partial-fp32s-bcols": ("persist_group_partial", "fp32s", dict(family=gc.SPLIT, np=3, persist=0)),
    "persist_513-beta_gate": ("persist_513", "beta_gate", {}),
    "tiled_group_partial-beta_gate": ("tiled_group_partial", "beta_gate", {}),
    "planes_split8-ones_col": ("planes_split8", "ones_col", {}),     # N = 501: still 8 column tiles
})


def _randn(*shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale).float()


@functools.lru_cache(maxsize=None)
def _inputs(run_id):
    """fp32 CPU inputs of a run, the same in every process: the logical A (batch, M, K) (a conv A: its (R, cin)
    source and its im2col value), B (batch, N, K), and the epilogue's operands."""
    case_id, variant, _ = RUNS[run_id]
    _, (M, N, K, batch, _), aform, bform, _ = CASES[case_id]
    seed = 1000 * sorted(RUNS).index(run_id)
    inp = {}
    if isinstance(aform, tuple):
        inp["a_src"] = _randn(M, gc.CONV_CIN, seed=seed + 1)
        inp["A"] = gc.im2col(inp["a_src"], aform[1], aform[2])[None]
    else:
        inp["A"] = _randn(batch, M, K, seed=seed + 1)
    # (ones_col: unit-variance rows as in test_gemm_fused_bias_column, whose tolerance it takes)
    inp["B"] = _randn(batch, N, K, seed=seed + 2, scale=1.0 if variant == "ones_col" else K ** -0.5)
    if variant in ("beta_gate", "ones_col"):
        inp["c0"] = _randn(batch, M, N, seed=seed + 3)
    if variant == "beta_gate":
        inp["gate"] = _randn(M, N, seed=seed + 4)
    if variant == "ones_col":
        inp["last0"] = _randn(M, seed=seed + 5)
    return inp


def _plain_operand(X, trans):
    """(batch, R, K) logical value -> (operand, device tensor): row-major as it is, column-major as (batch, K, R)."""
    t = (X.transpose(1, 2) if trans else X).contiguous().to(DEV)
    o = nx.Operand()
    o.ptr, o.ld, o.trans, o.conv_dir, o.batch_stride = nx.ptr(t), t.shape[-1], int(trans), 1, t[0].numel()
    return o, t


def _launch(run_id):
    """One fxf.gemm launch of the run: (C on the CPU, c_last on the CPU or None, the plan as a dict)."""
    from factmx import functional as fxf
    case_id, variant, _ = RUNS[run_id]
    _, (M, N, K, batch, split), aform, bform, _ = CASES[case_id]
    if variant == "fp32s":
        bform = "cols"
    inp = _inputs(run_id)
    if isinstance(aform, tuple):
        src = inp["a_src"].to(DEV)
        a = nx.Operand()
        a.ptr, a.ld, a.conv_dir = nx.ptr(src), gc.CONV_CIN, 1
        a.conv_taps, a.conv_cin, a.conv_dil, a.seq_len = 3, gc.CONV_CIN, aform[1], aform[2]
        keep = [src]
    else:
        a, ta = _plain_operand(inp["A"], aform == "cols")
        keep = [ta]
    b, tb = _plain_operand(inp["B"], bform == "cols")
    keep.append(tb)
    kw, c_last, Nd = {}, None, N
    if variant == "beta_gate":
        c = inp["c0"].to(DEV)
        gate = inp["gate"].to(DEV)
        kw = dict(beta=0.5, gate=gate)
    elif variant == "ones_col":
        Nd = N + 1
        b.ones_col = Nd
        c = inp["c0"].to(DEV)
        c_last = inp["last0"].to(DEV)
        kw = dict(beta=1.0, c_last=c_last)
    else:
        c = torch.full((batch, M, N), float("nan"), device=DEV)
    ws = torch.full((batch * split * M * Nd,), float("nan"), device=DEV) if split > 1 else None
    info = nx.GemmPlanInfo()
    with fxf.gemm_precision(variant if variant in gc.PRECS else "fp32"):
        fxf.gemm(M, Nd, K, a, b, c, N, split=split, batch=batch, c_bs=M * N, plan=info, ws=ws, **kw)
    torch.cuda.synchronize()
    return c.cpu(), None if c_last is None else c_last.cpu(), gc.plan_dict(info)


def _bad_tiles(bad, tile_m):
    """The (ty, tx) output tiles (tile_m x 64) of a (batch, M, N) mask that hold a set element."""
    idx = bad.nonzero()
    return sorted({(int(m) // tile_m, int(n) // 64) for _, m, n in idx.tolist()})


@pytest.mark.parametrize("run_id", list(RUNS))
def test_tile_order(run_id):
    case_id, variant, over = RUNS[run_id]
    _, (M, N, K, batch, split), aform, bform, want = CASES[case_id]
    c, c_last, plan = _launch(run_id)
    want = dict(want, **over)
    got = {k: plan[k] for k in want}
    assert got == want, (run_id, plan)                  # the plan first: the numbers below are about this path
    inp = _inputs(run_id)
    A, B = inp["A"].double(), inp["B"].double()
    ref = A @ B.transpose(1, 2)
    # the fp32 tolerance of tests/test_gpu_gemm.py
    tol = torch.full_like(ref, 1e-5 * (1 + ref.abs().max().item()) + 1e-6 * K ** 0.5)
    if variant == "bf16":   # plus the number format's bound, as test_gemm_family_pairs derives it
        tol = tol + ((1 + 2.0 ** -9) ** 2 - 1) * (A.abs() @ B.abs().transpose(1, 2))
    if variant == "beta_gate":
        ref = torch.where(inp["gate"].double() > 0, ref + 0.5 * inp["c0"].double(), torch.zeros_like(ref))
    if variant == "ones_col":   # test_gemm_fused_bias_column's: rtol 1e-5, atol max(1e-4, 5e-6 sqrt(K))
        ref = ref + inp["c0"].double()
        tol = max(1e-4, 5e-6 * K ** 0.5) + 1e-5 * ref.abs()
        ref_last = inp["last0"].double() + A[0].sum(1)
        err_last = (c_last.double() - ref_last).abs()
        bad_last = ~(err_last <= max(1e-4, 5e-6 * K ** 0.5) + 1e-5 * ref_last.abs())
        assert int(bad_last.sum()) == 0, (run_id, "c_last rows", bad_last.nonzero().flatten().tolist()[:32])
    err = (c.double() - ref).abs()
    bad = ~(err <= tol)                                 # NaN (an element no workgroup wrote) counts as bad
    nbad = int(bad.sum())
    tile_m = 128 if plan["family"] in (gc.WIDE8, gc.BF16, gc.SPLIT) else 64
    print(f"{run_id}: max err {err[~bad].max().item() if nbad < bad.numel() else float('nan'):.3e} "
          f"(tolerance from {tol.min().item():.3e}), {nbad} of {bad.numel()} elements bad, none excluded")
    if nbad:
        print(f"{run_id}: bad (ty, tx) tiles of {tile_m} x 64: {_bad_tiles(bad, tile_m)}; NaN: {int(c.isnan().sum())}")
    assert nbad == 0, (run_id, nbad)


def _child(path):
    """Knobs off (the parent set them in the environment): every run's output, after asserting the remaps off."""
    out = {}
    for run_id in RUNS:
        c, c_last, plan = _launch(run_id)
        assert all(not plan[r] for r in gc.REMAPS), (run_id, plan)
        out[run_id] = c
        out[run_id + "/plan"] = torch.tensor([plan[k] for k in ("family", "split", "tiles_x", "tiles_y")])
        if c_last is not None:
            out[run_id + "/c_last"] = c_last
    torch.save(out, path)


def test_tile_orders_bitwise_against_knobs_off(tmp_path):
    path = str(tmp_path / "knobs_off.pt")
    env = dict(os.environ, **gc.KNOBS_OFF)
    p = subprocess.run([sys.executable, "-u", os.path.abspath(__file__), path], env=env, cwd=_ROOT, timeout=240)
    assert p.returncode == 0, p.returncode
    off = torch.load(path, weights_only=True)
    on_fields = set()
    for run_id in RUNS:
        c, c_last, plan = _launch(run_id)
        on_fields |= {r for r in gc.REMAPS if plan[r] > (1 if r in ("row_perm", "group_m") else 0)}
        assert off[run_id + "/plan"].tolist() == [plan[k] for k in ("family", "split", "tiles_x", "tiles_y")], run_id
        assert not c.isnan().any(), run_id
        same = c == off[run_id]
        tile_m = 128 if plan["family"] in (gc.WIDE8, gc.BF16, gc.SPLIT) else 64
        assert bool(same.all()), (run_id, int((~same).sum()), _bad_tiles(~same, tile_m))
        if c_last is not None:
            assert torch.equal(c_last, off[run_id + "/c_last"]), run_id
    assert on_fields == set(gc.REMAPS)                  # (this process runs them)


if __name__ == "__main__":
    _child(sys.argv[1])
