"""Shared by tests/test_gemm_plan.py (no GPU) and tests/test_gpu_gemm_tiles.py: fx_gemm descriptors over made-up
addresses for the plan query fx_gemm_plan, and the shapes that put fx_gemm on each tile order of
block_tile / block_tile_id (csrc/gemm_dev.h) with the plan each one claims.

Run as a script it prints, as one JSON line, the plan of every TILE_CASES entry in this process -- the
library's knobs (FX_GEMM_XCDPLANES, FX_GEMM_ROWPERM, FX_GEMM_GROUPM, FX_GEMM_PERSIST) are read once per process,
so a test that wants them off asks a child."""
import ctypes
import json
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (_ROOT, os.path.join(_ROOT, "fact-clip_amd")):     # (a child process has no conftest)
    if _p not in sys.path:
        sys.path.insert(0, _p)

from factmx import native as nx  # noqa: E402

TILED, WIDE8, BF16, SPLIT, DIRECT = (nx.GEMM_FAM_TILED, nx.GEMM_FAM_WIDE8, nx.GEMM_FAM_BF16, nx.GEMM_FAM_SPLIT,
                                     nx.GEMM_FAM_DIRECT)
FAMILY_NAMES = {TILED: "tiled", WIDE8: "wide8", BF16: "bf16", SPLIT: "split", DIRECT: "direct"}
PRECS = {"fp32": nx.PREC_F32, "bf16": nx.PREC_BF16, "fp32s": nx.PREC_F32S, "fp32s2": nx.PREC_F32S2}
REMAPS = ("xcd_planes", "row_perm", "group_m", "persist")
KNOBS_OFF = {"FX_GEMM_XCDPLANES": "0", "FX_GEMM_ROWPERM": "0", "FX_GEMM_GROUPM": "0", "FX_GEMM_PERSIST": "0"}

# made-up, 16-byte aligned addresses: the planner tests pointers for NULL and alignment and never reads them
ADDR_A, ADDR_A1, ADDR_B, ADDR_B1, ADDR_POS, ADDR_C, ADDR_WS = (0x100000000000 * i for i in range(1, 8))
CONV_CIN = 64       # a conv A operand: 3 taps of 64 channels, K = 192


def fake_operand(form, R, K, addr, addr1=ADDR_A1, batch=1, dil=3, seq_len=None):
    """An fx_operand of R rows over K at a made-up address.  form: rows / cols (plain), conv (3-tap dilated conv:
    row-major when it is A, i.e. K == 3 cin; as B the column-major form with R == 3 cin), cat (two row-major
    sources split at k = 64), gen (rows plus a positional add); "+u" makes the leading dimension odd, so the
    operand is not 16-byte vector-loadable."""
    kind, _, flag = form.partition("+")
    u = int(flag == "u")
    o = nx.Operand()
    o.ptr, o.conv_dir = addr, 1
    if kind == "rows" or kind == "gen":
        o.ld, o.batch_stride = K + u, R * (K + u) if batch > 1 else 0
        if kind == "gen":
            o.pos, o.ld_pos, o.pos_cols = ADDR_POS, min(K, 40), min(K, 40)
    elif kind == "cols":
        o.ld, o.trans, o.batch_stride = R + u, 1, K * (R + u) if batch > 1 else 0
    elif kind == "cat":
        o.ld, o.ptr1, o.ld1, o.k_split = 64 + u, addr1, K - 64 + u, 64
    elif kind == "convA":
        o.ld, o.conv_taps, o.conv_cin, o.conv_dil, o.seq_len = K // 3 + u, 3, K // 3, dil, seq_len or R
    elif kind == "convB":
        o.ld, o.trans, o.conv_taps, o.conv_cin, o.conv_dil, o.seq_len = R // 3 + u, 1, 3, R // 3, dil, seq_len or K
    else:
        raise AssertionError(form)
    return o


def fake_desc(M, N, K, batch=1, split=1, a="rows", b="rows", **fields):
    """fx_gemm_desc over made-up addresses; a / b: a fake_operand form (conv: convA / convB by side) or an
    nx.Operand; fields: further descriptor fields by name."""
    d = nx.GemmDesc()
    d.M, d.N, d.K, d.batch = M, N, K, batch
    if isinstance(a, str):
        a = fake_operand(a.replace("conv", "convA"), M, K, ADDR_A, ADDR_A1, batch)
    if isinstance(b, str):
        b = fake_operand(b.replace("conv", "convB"), N, K, ADDR_B, ADDR_B1, batch)
    d.a, d.b = a, b
    d.c, d.ldc, d.c_batch_stride, d.alpha, d.split_k = ADDR_C, N, M * N if batch > 1 else 0, 1.0, split
    if split > 1:
        d.workspace = ADDR_WS
    for k, v in fields.items():
        setattr(d, k, v)
    return d


def plan_of(desc, prec="fp32"):
    """(status, nx.GemmPlanInfo) of fx_gemm_plan."""
    info = nx.GemmPlanInfo()
    st = nx.load().fx_gemm_plan(ctypes.byref(desc), PRECS[prec], ctypes.byref(info))
    return st, info


def plan_dict(info):
    return {n: getattr(info, n) for n, _ in info._fields_}


def conv_a(dil, seq_len):
    return ("conv", dil, seq_len)


# ---------------------------------------------------------------- the tile-order cases
# id, (M, N, K, batch, split), A form, B form, the plan the case stands on.  A conv A is ("conv", dil, seq_len)
# with cin 64.  Wide tiles are 128 x 64, tiled ones 64 x 64; `want` names the remap field the case is about and
# leaves the others to the knobs-off comparison.
TILE_CASES = [
    # persist (gemm_plan.cpp "FX_GEMM_PERSIST"): >= 512 tiles, walked by a grid of 256 workgroups
    ("persist_513", (3400, 1200, 128, 1, 1), "rows", "rows",      # 513 = 2 * 256 + 1: one workgroup takes a third tile
     dict(family=WIDE8, split=1, tiles_x=19, tiles_y=27, persist=513, grid_x=256)),
    ("persist_512", (4096, 1024, 128, 1, 1), "rows", "rows",      # at the threshold
     dict(family=WIDE8, split=1, tiles_x=16, tiles_y=32, persist=512, grid_x=256)),
    ("persist_off_496", (3968, 1024, 128, 1, 1), "rows", "rows",  # one row tile below it
     dict(family=WIDE8, split=1, tiles_x=16, tiles_y=31, persist=0, grid_x=16)),
    ("persist_group_partial", (3662, 1200, 512, 1, 1), "rows", "rows",   # 29 row tiles in groups of 3: the last has 2
     dict(family=WIDE8, split=1, tiles_x=19, tiles_y=29, persist=551, group_m=3)),
    # group_m ("FX_GEMM_GROUPM"): >= 16 x 8 tiles, B over 2 MB, one run of A rows at most 2 MB
    ("tiled_group_partial", (1160, 520, 1088, 1, 1), "rows", "rows",     # 19 row tiles in groups of 2: the last has 1
     dict(family=TILED, split=1, tiles_x=9, tiles_y=19, group_m=2, fast=1)),
    ("tiled_group_off", (1160, 520, 1008, 1, 1), "rows", "rows",  # B = 520 x 1008 x 4 B, 512 B under 2 MB; K % 64 = 48
     dict(family=TILED, split=1, tiles_x=9, tiles_y=19, group_m=0, fast=0)),    # is a K tail on the generic loop
    # xcd_planes ("FX_GEMM_XCDPLANES"): wide launches of a multiple of 8 z-planes (batch x split)
    ("planes_batch8", (300, 500, 128, 8, 1), "rows", "rows",
     dict(family=WIDE8, split=1, tiles_x=8, tiles_y=3, grid_z=8, xcd_planes=1)),
    ("planes_batch16", (200, 500, 128, 16, 1), "rows", "rows",
     dict(family=WIDE8, split=1, tiles_x=8, tiles_y=2, grid_z=16, xcd_planes=1)),
    ("planes_split8", (300, 500, 4096, 1, 8), "cols", "cols",
     dict(family=WIDE8, split=8, tiles_x=8, tiles_y=3, grid_z=8, xcd_planes=1, in_launch_reduce=0)),
    ("planes_batch2_split4_ktail", (300, 500, 2500, 2, 4), "cols", "cols",
     dict(family=WIDE8, split=4, tiles_x=8, tiles_y=3, grid_z=8, xcd_planes=1, a_kind=nx.GEMM_KIND_COLS_KT,
          b_kind=nx.GEMM_KIND_COLS_KT)),
    ("planes_24", (300, 500, 4096, 3, 8), "cols", "cols",
     dict(family=WIDE8, split=8, tiles_x=8, tiles_y=3, grid_z=24, xcd_planes=1)),
    ("planes_off_split7", (300, 500, 2112, 1, 8), "cols", "cols",     # 33 stages in 8: 5 per slice, 7 slices: not wide
     dict(family=TILED, split=7, tiles_x=8, tiles_y=5, grid_z=7, xcd_planes=0)),
    ("planes_off_12", (300, 500, 4096, 3, 4), "cols", "cols",
     dict(family=WIDE8, split=4, tiles_x=8, tiles_y=3, grid_z=12, xcd_planes=0)),
    # row_perm ("FX_GEMM_ROWPERM"): dilated-conv A shifting by dil / 128 whole row tiles that divide the row tiles
    ("row_perm_2", (2000, 768, 192, 1, 1), conv_a(256, 1000), "rows",     # 16 row tiles, the last 80 rows short
     dict(family=WIDE8, split=1, tiles_x=12, tiles_y=16, row_perm=2)),
    ("row_perm_3", (2250, 768, 192, 1, 1), conv_a(384, 1125), "rows",
     dict(family=WIDE8, split=1, tiles_x=12, tiles_y=18, row_perm=3)),
    ("row_perm_off_17", (2176, 768, 192, 1, 1), conv_a(256, 1088), "rows",   # 17 % 2 != 0
     dict(family=WIDE8, split=1, tiles_x=12, tiles_y=17, row_perm=0)),
    # the 64 x 64 kernel's in-launch split-K reduction (2 slabs of a tile = 32 KB, the most the planner keeps)
    ("tiled_in_launch_reduce", (600, 520, 3000, 1, 2), "cols", "rows",
     dict(family=TILED, split=2, tiles_x=9, tiles_y=10, in_launch_reduce=1)),
]
TILE_CASE_IDS = [c[0] for c in TILE_CASES]


def tile_case_desc(case, ones_col=False):
    """The case's descriptor over made-up addresses (ones_col: B with the virtual ones column, N + 1 columns)."""
    _, (M, N, K, batch, split), a, b, _ = case
    if isinstance(a, tuple):
        a = fake_operand("convA", M, K, ADDR_A, dil=a[1], seq_len=a[2])
    if ones_col:
        b = fake_operand(b, N, K, ADDR_B, ADDR_B1, batch)
        b.ones_col = N + 1
        return fake_desc(M, N + 1, K, batch, split, a, b, ldc=N, c_last_col=ADDR_POS, beta=1.0)
    return fake_desc(M, N, K, batch, split, a, b)


def check_plan(info, want, what):
    got = {k: getattr(info, k) for k in want}
    assert got == want, (what, got, want)


def im2col(X, dil, seq_len):
    """(R, cin) -> (R, 3 cin): column j cin + c of row r is X[r + (j - 1) dil, c], zero outside r's video."""
    import torch
    R, cin = X.shape
    out = torch.zeros(R, 3 * cin, dtype=X.dtype)
    for s in range(0, R, seq_len):
        e = min(R, s + seq_len)
        for j in range(3):
            sh = (j - 1) * dil
            lo, hi = max(s, s - sh), min(e, e - sh)
            if hi > lo:
                out[lo:hi, j * cin:(j + 1) * cin] = X[lo + sh:hi + sh]
    return out


if __name__ == "__main__":
    plans = {}
    for case in TILE_CASES:
        st, info = plan_of(tile_case_desc(case))
        plans[case[0]] = dict(plan_dict(info), status=st)
    print(json.dumps(plans))
