"""fx_gemm_plan: every launch decision of the GEMM planner (csrc/gemm_plan.cpp), both sides of each threshold,
asked of the library without a GPU.  The descriptors hold made-up, 16-byte aligned addresses: the planner
tests operand pointers for NULL and alignment and never reads through them, and nothing is allocated.

Each test names the rule of gemm_plan.cpp it stands on (use_direct, its `fits` guard, use_wide, the split
arithmetic and the slab bound of plan_gemm, the family choice, the four tile-order blocks after the knob
comments).  The numbers in the comments restate the rule for the shape at hand."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

import gemm_cases as gc
from factmx import native as nx
from gemm_cases import BF16, DIRECT, SPLIT, TILED, WIDE8, fake_desc, fake_operand, plan_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_SHAPE, ERR_UNSUPPORTED = -1, -3


@pytest.fixture(scope="module")
def lib():
    return nx.load()


def plan(*args, prec="fp32", **kw):
    """The plan of fake_desc(*args, **kw); the query must succeed."""
    st, info = plan_of(fake_desc(*args, **kw), prec)
    assert st == 0, (st, nx.load().fx_last_error())
    return info


def family(*args, **kw):
    return plan(*args, **kw).family


# ---------------------------------------------------------------- the query itself
def test_query_contract(lib):
    assert lib.fx_version() == 30 == nx.ABI_VERSION
    assert lib.fx_struct_size(8) == ctypes.sizeof(nx.GemmPlanInfo) == 18 * 4
    info = nx.GemmPlanInfo()
    info.family = info.persist = 77
    # an empty product plans nothing, as fx_gemm launches nothing -- before the operands are looked at
    st, info0 = plan_of(nx.GemmDesc(M=0, N=8, K=8, batch=1))
    assert st == 0 and not any(gc.plan_dict(info0).values())
    d = fake_desc(0, 8, 8)
    assert lib.fx_gemm_plan(ctypes.byref(d), nx.PREC_F32, ctypes.byref(info)) == 0
    assert not any(gc.plan_dict(info).values())            # ... and the output is zeroed, not left
    d = fake_desc(8, 0, 8)
    assert lib.fx_gemm_plan(ctypes.byref(d), nx.PREC_F32, ctypes.byref(info)) == 0
    # what fx_gemm refuses, the query refuses with the same status and text
    st, _ = plan_of(nx.GemmDesc(M=8, N=8, K=8, batch=1))
    assert st == ERR_SHAPE and b"null operand" in lib.fx_last_error()
    st, _ = plan_of(fake_desc(8, 8, 8, batch=0))
    assert st == ERR_SHAPE and b"bad sizes" in lib.fx_last_error()
    d = fake_desc(8, 8, 8)
    assert lib.fx_gemm_plan(ctypes.byref(d), nx.PREC_DEFAULT, ctypes.byref(info)) == ERR_SHAPE   # a stream's own precision only
    assert lib.fx_gemm_plan(ctypes.byref(d), 4, ctypes.byref(info)) == ERR_SHAPE
    assert lib.fx_gemm_plan(None, nx.PREC_F32, ctypes.byref(info)) == ERR_SHAPE
    assert lib.fx_gemm_plan(ctypes.byref(d), nx.PREC_F32, None) == ERR_SHAPE


def test_grid_and_block(lib):
    p = plan(32, 512, 512)                                   # direct: 32 x 32 tiles, one wave per 32-deep chunk, <= 8
    assert (p.family, p.tiles_x, p.tiles_y, p.block) == (DIRECT, 16, 1, 512)
    assert (p.grid_x, p.grid_y, p.grid_z) == (16, 1, 1)
    p = plan(32, 512, 96)
    assert (p.family, p.block) == (DIRECT, 3 * 64)
    p = plan(1000, 700, 128, batch=2)                        # tiled: 64 x 64 tiles, z = batch x split
    assert (p.family, p.tiles_x, p.tiles_y, p.block) == (TILED, 11, 16, 256)
    assert (p.grid_x, p.grid_y, p.grid_z) == (11, 16, 2)
    p = plan(1500, 1000, 128)                                # wide: 128 x 64 tiles, 8 waves
    assert (p.family, p.tiles_x, p.tiles_y, p.block) == (WIDE8, 16, 12, 512)


# ---------------------------------------------------------------- use_direct
def test_direct_by_token_rows():
    """`d.M <= lim || d.N <= lim` with lim 64 for plain operands.  K = 4096 keeps the shallow-K and few-tile
    rules out of the way (K > 2048)."""
    assert family(64, 1000, 4096) == DIRECT and family(65, 1000, 4096) == TILED
    assert family(1000, 64, 4096) == DIRECT and family(1000, 65, 4096) == TILED
    assert family(64, 1000, 4096, a="cols", b="cols") == DIRECT
    assert family(65, 1000, 4096, a="cols", b="cols") == TILED


@pytest.mark.parametrize("aform", ["cat", "gen"])
def test_direct_by_token_rows_gathered_a(aform):
    """lim is 32 for a concatenated (ptr1) or positional (pos) A: ROWS_CAT / ROWS_GEN load element by element."""
    assert family(32, 1000, 4096, a=aform) == DIRECT
    assert family(33, 1000, 4096, a=aform) == TILED
    assert family(33, 1000, 4096, a="rows") == DIRECT        # (the plain operand's limit is still 64)
    assert family(1000, 32, 4096, a=aform) == DIRECT and family(1000, 33, 4096, a=aform) == TILED


def test_direct_by_shallow_k():
    """`d.K <= 64 || (d.K <= 512 && d.K % 64 != 0)` at 1000 x 1000: 1024 tiles of 32 x 32, over the few-tile rule."""
    assert family(1000, 1000, 64) == DIRECT and family(1000, 1000, 128) == TILED
    assert family(1000, 1000, 448) == TILED                  # whole 64-deep stages: the FAST tiled loop
    assert family(1000, 1000, 449) == DIRECT                 # a K tail at K <= 512
    assert family(1000, 1000, 511) == DIRECT
    assert family(1000, 1000, 513) == TILED                  # past 512 the K tail takes the generic tiled loop
    assert plan(1000, 1000, 448).fast == 1 and plan(1000, 1000, 513).fast == 0


def test_direct_by_few_tiles():
    """`t32 <= 512 && d.K <= 2048` for plain operands, t32 = cdiv(M, 32) cdiv(N, 32) batch."""
    assert family(512, 1024, 128) == DIRECT                  # 16 x 32 = 512
    assert family(512, 1025, 128) == TILED                   # 16 x 33 = 528
    assert family(513, 1024, 128) == TILED                   # 17 x 32
    assert family(256, 1024, 128, batch=2) == DIRECT and family(256, 1025, 128, batch=2) == TILED
    assert family(512, 1024, 2048) == DIRECT and family(512, 1024, 2049) == TILED
    assert family(512, 1024, 128, a="cols", b="cols") == DIRECT
    assert family(512, 1024, 128, a="cat") == TILED          # (ak == ROWS || ak == COLS) only
    assert family(512, 1024, 128, a="gen") == TILED


def test_conv_and_dilation_growth_are_never_direct():
    """direct_pair has no conv kind; `d.b_dil_growth <= 1 && d.a_dil_b1 <= 0` guards use_direct."""
    assert family(32, 96, 192, a="conv") == TILED            # 32 token rows, still tiled
    assert family(32, 96, 128, b="conv") == TILED
    assert family(32, 96, 128, a="cols", b="conv") == TILED
    assert family(32, 96, 128, batch=2, b="conv", b_dil_growth=2) == TILED
    assert family(32, 96, 192, batch=2, a="conv", a_dil_b1=5) == TILED
    assert family(32, 96, 128) == DIRECT                     # the same shape on plain operands


def test_direct_needs_32_bit_offsets():
    """`fits`: the direct kernel addresses a ROWS operand of R rows within (R ld + K + 2 * 8 * 32 + 64) * 4 < 2^32
    bytes.  R = 32, K = 128: 32 ld + 704 < 2^30, so ld <= 33554409.  Only the number is planned: no memory."""
    def fam(ld_a=128, ld_b=128, bform="rows"):
        a = fake_operand("rows", 32, 128, gc.ADDR_A)
        a.ld = ld_a
        b = fake_operand(bform, 512, 128, gc.ADDR_B)
        b.ld = ld_b
        return family(32, 512, 128, a=a, b=b)
    assert fam() == DIRECT
    assert fam(ld_a=2 ** 25) == TILED                        # 32 x 2^25 x 4 B = 2^32
    assert fam(ld_a=33554409) == DIRECT and fam(ld_a=33554410) == TILED
    # B, 512 rows: 512 ld + 704 < 2^30 -> ld <= 2097150; as COLS (k ld + R) 4: 704 ld + 512 < 2^30 -> ld <= 1525200
    assert fam(ld_b=2097150) == DIRECT and fam(ld_b=2097151) == TILED
    assert fam(ld_b=1525200, bform="cols") == DIRECT and fam(ld_b=1525201, bform="cols") == TILED


# ---------------------------------------------------------------- use_wide
def test_wide_from_192_wide_tiles():
    """`cdiv(M, 128) * tiles_x * batch * split >= 192` (tiles_x of 64 columns)."""
    assert family(1536, 1024, 128) == WIDE8                  # 12 x 16 = 192
    assert family(1408, 1024, 128) == TILED                  # 11 x 16 = 176
    assert family(1409, 1024, 128) == WIDE8                  # cdiv: 12 row tiles
    assert family(768, 1024, 128) == TILED                   # 6 x 16 = 96 ...
    assert family(768, 1024, 128, batch=2) == WIDE8          # ... x 2 batches
    assert family(768, 1024, 128, split=2) == WIDE8          # ... x 2 K slices
    assert family(768, 960, 128, split=2) == TILED           # 6 x 15 x 2 = 180
    # 191 is prime: one factor must be tiles_x = 1, i.e. N <= 64, which only a conv operand keeps off the direct kernel
    assert family(191 * 128, 48, 128, b="conv") == TILED
    assert family(191 * 128 + 1, 48, 128, b="conv") == WIDE8


def test_wide_needs_fast_operands():
    """`fast = a_vec && b_vec && (K % 64 == 0 || ak == COLS_KT)` and wide8_pair."""
    p = plan(1536, 1024, 520, b="cols")                      # rows x cols, K % 64 = 8: the generic 64 x 64 loop
    assert (p.family, p.fast) == (TILED, 0)
    p = plan(1536, 1024, 520, a="cols", b="cols")            # cols x cols, same K: the K-tail kinds stay eligible
    assert (p.family, p.a_kind, p.b_kind) == (WIDE8, nx.GEMM_KIND_COLS_KT, nx.GEMM_KIND_COLS_KT)
    assert family(1536, 1024, 512, b="cols") == WIDE8
    for kw in (dict(a="rows+u"), dict(b="rows+u"), dict(a="cols+u", b="cols"), dict(a="cols", b="cols+u")):
        p = plan(1536, 1024, 128, **kw)
        assert (p.family, p.fast) == (TILED, 0), kw
    a = fake_operand("rows", 1536, 128, gc.ADDR_A + 4)       # an address off by one float
    assert family(1536, 1024, 128, a=a) == TILED
    assert family(1536, 1024, 128, a="gen") == TILED         # a positional add: no FAST loader
    # an unaligned cols x cols K tail keeps plain COLS kinds on the generic loop
    p = plan(1536, 1024, 520, a="cols+u", b="cols")
    assert (p.family, p.a_kind, p.b_kind) == (TILED, nx.GEMM_KIND_COLS, nx.GEMM_KIND_COLS)


# ---------------------------------------------------------------- split
def test_tiled_split_arithmetic():
    """`split = min(cap, nkt); kt_per_split = cdiv(nkt, split); split = cdiv(nkt, kt_per_split)`, nkt = cdiv(K, 64)."""
    p = plan(300, 500, 2112, split=8, a="cols", b="cols")    # 33 stages, cap 8: 5 per slice -> 7 slices
    assert (p.family, p.split, p.kt_per_split, p.grid_z) == (TILED, 7, 5, 7)
    p = plan(1000, 1000, 128, split=8)                       # a cap above nkt = 2 clamps to it
    assert (p.split, p.kt_per_split) == (2, 1)
    p = plan(1000, 1000, 4096, split=8)                      # 64 stages in 8
    assert (p.split, p.kt_per_split) == (8, 8)
    p = plan(1000, 1000, 4097, split=8)                      # 65 stages: 9 per slice, 8 slices (the last has 2)
    assert (p.split, p.kt_per_split) == (8, 9)
    p = plan(1000, 1000, 4096, split=13, batch=2)            # 64 in 13: 5 per slice -> 13; z = batch x split
    assert (p.split, p.kt_per_split, p.grid_z) == (13, 5, 26)
    p = plan(1000, 1000, 4096, split=12)                     # 64 in 12: 6 per slice -> 11 slices
    assert (p.split, p.kt_per_split) == (11, 6)


def test_direct_split_rule():
    """Direct: split only when `cap > 1 && t32 < 64`, `want = min(nch / nw, cdiv(2048, t32 * nw))`, nch = cdiv(K, 32)
    chunks on nw = min(8, nch) waves."""
    p = plan(32, 256, 1024, split=4, b="cols")               # t32 = 8, nch = 32: want = min(4, 32) = 4
    assert (p.family, p.split, p.kt_per_split) == (DIRECT, 4, 8)
    assert plan(32, 256, 1024, split=16, b="cols").split == 4        # the cap does not raise `want`
    assert plan(32, 256, 1024, split=3, b="cols").split == 3         # ... and bounds it: cdiv(32, 3) = 11 -> 3 slices
    p = plan(32, 2016, 4096, split=32)                       # t32 = 63: want = min(128 / 8, cdiv(2048, 504) = 5)
    assert (p.family, p.split, p.kt_per_split) == (DIRECT, 5, 26)
    p = plan(32, 2048, 4096, split=32)                       # t32 = 64: unsplit
    assert (p.family, p.split) == (DIRECT, 1)
    p = plan(32, 32, 4096, batch=8, split=32, b="cols")      # t32 = 8: want = min(16, 32)
    assert (p.family, p.split, p.grid_z) == (DIRECT, 16, 128)
    assert plan(32, 256, 128, split=4).split == 1            # nch / nw = 4 / 4 = 1: nothing to split


def test_split_needs_a_workspace(lib):
    d = fake_desc(1000, 1000, 4096, split=8)
    d.workspace = None
    st, _ = plan_of(d)
    assert st == ERR_SHAPE and b"split-K needs a workspace" in lib.fx_last_error()
    d.split_k = 1
    assert plan_of(d)[0] == 0


def test_in_launch_reduction():
    """`slab_bytes = split * tile * 4 <= 32768` keeps the last arriver's reduction inside the launch."""
    p = plan(600, 520, 3000, split=2, a="cols")              # 64 x 64 tile: 2 x 16 KB
    assert (p.family, p.split, p.in_launch_reduce) == (TILED, 2, 1)
    p = plan(600, 520, 3000, split=3, a="cols")
    assert (p.family, p.split, p.in_launch_reduce) == (TILED, 3, 0)
    assert plan(600, 520, 3000, a="cols").in_launch_reduce == 0      # nothing to reduce
    for split in (2, 4, 8):                                  # 128 x 64 tile: 2 x 32 KB already over
        p = plan(1536, 1024, 4096, split=split)
        assert (p.family, p.split, p.in_launch_reduce) == (WIDE8, split, 0)
    for cap, want in ((2, 1), (8, 1), (16, 0)):              # 32 x 32 tile: up to 8 x 4 KB
        p = plan(32, 32, 4096, split=cap, b="cols")
        assert (p.family, p.split, p.in_launch_reduce) == (DIRECT, cap, want)
    # one arrival counter per output tile: 65536 of them (kArrivalCounters)
    assert plan(6400, 6400, 128, split=2).family == WIDE8
    p = plan(16384, 16384, 128, split=2, a="rows+u")         # 256 x 256 = 65536 tiles of 64 x 64
    assert (p.family, p.in_launch_reduce) == (TILED, 1)
    p = plan(16385, 16384, 128, split=2, a="rows+u")
    assert (p.family, p.in_launch_reduce) == (TILED, 0)


# ---------------------------------------------------------------- the family under the precision modes
@pytest.mark.parametrize("aform", ["rows", "conv", "cat"])
def test_precision_families_rowmajor_a(aform):
    """`lowp = wide && bf16_pair(ak, bk)`: row-major A against B rows / cols on a wide launch."""
    K = 192 if aform == "conv" else 128
    for prec, want_rows, want_cols in (("fp32", (WIDE8, 0), (WIDE8, 0)), ("bf16", (BF16, 0), (BF16, 0)),
                                       ("fp32s", (WIDE8, 3), (SPLIT, 3)), ("fp32s2", (WIDE8, 2), (SPLIT, 2))):
        p = plan(1536, 1024, K, a=aform, b="rows", prec=prec)
        assert (p.family, p.np) == want_rows, (prec, "rows")
        p = plan(1536, 1024, K, a=aform, b="cols", prec=prec)
        assert (p.family, p.np) == want_cols, (prec, "cols")


@pytest.mark.parametrize("prec", ["bf16", "fp32s", "fp32s2"])
def test_precision_modes_elsewhere_keep_f32(prec):
    for b in ("rows", "cols"):                               # weight gradients (column-major A) keep the f32 MFMA
        p = plan(1536, 1024, 128, a="cols", b=b, prec=prec)
        assert (p.family, p.np) == (WIDE8, 0)
    p = plan(1536, 1008, 128, b="conv", prec=prec)           # a conv B is outside bf16_pair
    assert (p.family, p.np) == (WIDE8, 0)
    for b in ("rows", "cols"):                               # not wide: the 64 x 64 and direct kernels as they are
        p = plan(768, 768, 128, b=b, prec=prec)
        assert (p.family, p.np) == (TILED, 0)
        p = plan(32, 96, 128, b=b, prec=prec)
        assert (p.family, p.np) == (DIRECT, 0)


# ---------------------------------------------------------------- the tile orders
@pytest.mark.parametrize("case", gc.TILE_CASES, ids=gc.TILE_CASE_IDS)
def test_tile_case_plans(case):
    """The on / off pairs that tests/test_gpu_gemm_tiles.py launches."""
    st, info = plan_of(gc.tile_case_desc(case))
    assert st == 0
    gc.check_plan(info, case[4], case[0])


def test_persist_conditions():
    """`family == FAM_WIDE8 && !np && split == 1 && batch == 1 && !xcd_planes`, `nt >= 2 * 256`."""
    assert plan(4096, 1024, 128).persist == 512
    assert plan(4096, 1024, 128).group_m == 0                # (B is 512 KB)
    p = plan(4096, 1024, 128, batch=2)
    assert (p.family, p.persist, p.grid_z) == (WIDE8, 0, 2)
    p = plan(4096, 1024, 128, split=2)
    assert (p.family, p.split, p.persist) == (WIDE8, 2, 0)
    p = plan(4096, 1024, 128, batch=8)                       # planes instead
    assert (p.xcd_planes, p.persist) == (1, 0)
    for prec, fam in (("bf16", BF16), ("fp32s", WIDE8), ("fp32s2", WIDE8)):
        p = plan(4096, 1024, 128, prec=prec)
        assert (p.family, p.persist, p.grid_x, p.grid_y) == (fam, 0, 16, 32), prec
    p = plan(4096, 1024, 128, b="cols", prec="fp32s")
    assert (p.family, p.persist) == (SPLIT, 0)
    assert plan(4096, 1024, 128, a="cols", prec="bf16").persist == 512   # a weight gradient keeps the f32 kernel
    assert plan(8192, 1024, 128, a="rows+u").persist == 0    # 2048 tiles on the 64 x 64 kernel


def test_group_m_conditions():
    """`tiles_y >= 16 && tiles_x >= 8`, plain operands, `b_bytes > 2 MB && a_run <= 2 MB` with a_run the
    tiles_y / 8 row tiles of one XCD run."""
    assert plan(2048, 2752, 192).group_m == 2                # 16 row tiles; B = 2752 x 192 x 4 = 2113536 B
    assert plan(2048, 2752, 192, a="conv").group_m == 0      # a conv operand (dilation 3: no row permutation)
    assert plan(2048, 2752, 192, a="conv").row_perm == 0
    assert plan(2048, 2736, 192, b="conv").group_m == 0
    assert plan(2048, 2728, 192).group_m == 0                # B = 2095104 B, under 2 MB
    assert plan(1920, 2752, 192).group_m == 0                # 15 row tiles
    assert plan(2048, 2752, 192, b="cols").group_m == 2
    p = plan(8192, 1200, 512)                                # 64 row tiles: runs of 8 x 128 rows x 512 x 4 B = 2 MB
    assert (p.family, p.group_m) == (WIDE8, 8)
    assert plan(8192, 1200, 576).group_m == 0                # ... x 576: over
    p = plan(2048, 448, 1280)                                # 7 column tiles (B = 2.2 MB), 32 row tiles of 64
    assert (p.family, p.tiles_x, p.tiles_y, p.group_m) == (TILED, 7, 32, 0)
    assert plan(2048, 449, 1280).group_m == 4                # 8 column tiles; runs of 4 x 64 rows x 1280 x 4 B
    assert plan(1160, 520, 1088).group_m == 2 and plan(1160, 520, 1008).group_m == 0
    assert plan(2048, 2752, 192, batch=8).group_m == 0       # planes take precedence
    assert plan(2048, 2752, 192, batch=8).xcd_planes == 1


def test_row_perm_conditions():
    """`sh = conv_dil / 128; sh > 1 && tiles_y % sh == 0`, wide launches with a row-major 3-tap conv A."""
    def rp(M, dil, seq_len, **kw):
        return plan(M, 768, 192, a=fake_operand("convA", M, 192, gc.ADDR_A, dil=dil, seq_len=seq_len), **kw)
    assert rp(2048, 256, 1024).row_perm == 2
    assert rp(2048, 255, 1024).row_perm == 0                 # 255 / 128 = 1: the taps stay within a neighbour tile
    assert rp(2048, 128, 1024).row_perm == 0
    assert rp(2048, 384, 1024).row_perm == 0                 # 16 % 3
    assert rp(2304, 384, 1152).row_perm == 3
    assert rp(2176, 256, 1088).row_perm == 0                 # 17 % 2
    assert rp(2048, 256, 1024, a_dil_b1=512, batch=2).row_perm == 0      # a second dilation in the launch
    p = rp(2048, 256, 1024, batch=8)                         # planes take precedence
    assert (p.xcd_planes, p.row_perm) == (1, 0)
    p = plan(1024, 768, 192, a=fake_operand("convA", 1024, 192, gc.ADDR_A, dil=256, seq_len=512))
    assert (p.family, p.row_perm) == (TILED, 0)              # 8 x 12 = 96 wide tiles: not wide


def test_xcd_planes_conditions():
    """`wide && nz >= 8 && nz % 8 == 0`, nz = batch x split."""
    assert plan(300, 500, 128, batch=8).xcd_planes == 1
    assert plan(300, 500, 128, batch=7).xcd_planes == 0      # 3 x 8 x 7 = 168 wide tiles: tiled anyway
    assert plan(300, 500, 128, batch=9).xcd_planes == 0 and family(300, 500, 128, batch=9) == WIDE8
    assert plan(300, 500, 4096, batch=3, split=4, a="cols", b="cols").xcd_planes == 0      # 12 planes
    assert plan(300, 500, 4096, batch=3, split=8, a="cols", b="cols").xcd_planes == 1      # 24
    assert plan(300, 500, 4096, batch=4, split=4, a="cols", b="cols").xcd_planes == 1      # 16
    p = plan(300, 500, 128, batch=8, a="rows+u")             # 64 x 64 kernel: no planes
    assert (p.family, p.xcd_planes) == (TILED, 0)


def test_knobs_off_in_a_child_process(lib):
    """FX_GEMM_XCDPLANES / ROWPERM / GROUPM / PERSIST = 0 (read once per process): every tile order off, the
    same kernel, split and tiles; persist gives the grid back to one workgroup per tile."""
    env = dict(os.environ, **gc.KNOBS_OFF)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gemm_cases.py")], env=env, cwd=ROOT,
                         capture_output=True, text=True, timeout=120, check=True)
    child = json.loads(out.stdout.strip().splitlines()[-1])
    assert set(child) == set(gc.TILE_CASE_IDS)
    some_on = set()
    for case in gc.TILE_CASES:
        st, info = plan_of(gc.tile_case_desc(case))
        mine, theirs = gc.plan_dict(info), child[case[0]]
        assert st == 0 and theirs["status"] == 0
        assert all(not theirs[r] for r in gc.REMAPS), (case[0], theirs)
        for k in ("family", "a_kind", "b_kind", "fast", "np", "split", "kt_per_split", "tiles_x", "tiles_y", "block",
                  "in_launch_reduce"):
            assert mine[k] == theirs[k], (case[0], k)
        assert (theirs["grid_x"], theirs["grid_y"], theirs["grid_z"]) == (
            mine["tiles_x"], mine["tiles_y"], mine["grid_z"]), case[0]
        some_on |= {r for r in gc.REMAPS if mine[r] > (1 if r in ("row_perm", "group_m") else 0)}
    assert some_on == set(gc.REMAPS)                         # (this process has them on)


# ---------------------------------------------------------------- the kind table
KINDS = ["ROWS", "ROWS_CONV", "ROWS_GEN", "COLS", "COLS_CONV", "ROWS_CAT", "COLS_CONVR", "COLS_KT"]
ROWS, ROWS_CONV, ROWS_GEN, COLS, COLS_CONV, ROWS_CAT, COLS_CONVR, COLS_KT = range(8)


# the families' pair predicates, restated from csrc/gemm_plan.h
def gen_kind(k):
    return ROWS_GEN if k == ROWS_CAT else k


def rowmajor_a(ak):
    return ak in (ROWS, ROWS_CONV, ROWS_CAT)


def tiled_pair(ak, bk, fast):
    a = rowmajor_a(ak) or ak in (COLS, COLS_KT) or (ak == ROWS_GEN and not fast)
    b = bk in (ROWS, COLS, COLS_CONV) or (bk == ROWS_GEN and not fast) or (
        fast and ((bk == COLS_CONVR and ak == COLS) or (bk == COLS_KT and ak == COLS_KT)))
    return a and b


def family_accepts(p):
    ak, bk = p.a_kind, p.b_kind
    if p.family == DIRECT:
        return gen_kind(ak) in (ROWS, ROWS_GEN, COLS) and bk in (ROWS, COLS)
    if p.family == TILED:
        return tiled_pair(ak, gen_kind(bk), bool(p.fast))
    if p.family == BF16:
        return rowmajor_a(ak) and bk in (ROWS, COLS)
    if p.family == SPLIT:
        return rowmajor_a(ak) and bk == COLS
    if p.family == WIDE8:
        return (rowmajor_a(ak) and bk == ROWS) if p.np else tiled_pair(ak, bk, True)
    return False


A_FORMS, B_FORMS = ("rows", "cols", "conv", "cat", "gen"), ("rows", "cols", "conv", "gen")
SHAPES = {"SMALL": (32, 96), "TILED": (768, 768), "WIDE": (1536, 1024)}     # as tests/test_gpu_gemm.py names them

# (shape class, which operand is unaligned) -> one row per A form in A_FORMS order, one entry per B form in
# B_FORMS order: "family:A kind/B kind", a * after the family for the 64 x 64 kernel's FAST loaders.  fp32.
_GEN4 = ["tiled:ROWS_GEN/ROWS", "tiled:ROWS_GEN/COLS", "tiled:ROWS_GEN/COLS_CONV", "tiled:ROWS_GEN/ROWS_GEN"]
_DGEN4 = ["direct:ROWS_GEN/ROWS", "direct:ROWS_GEN/COLS", "tiled:ROWS_GEN/COLS_CONV", "tiled:ROWS_GEN/ROWS_GEN"]
_GENERIC = [["tiled:ROWS/ROWS", "tiled:ROWS/COLS", "tiled:ROWS/COLS_CONV", "tiled:ROWS/ROWS_GEN"],
            ["tiled:COLS/ROWS", "tiled:COLS/COLS", "tiled:COLS/COLS_CONV", "tiled:COLS/ROWS_GEN"],
            ["tiled:ROWS_CONV/ROWS", "tiled:ROWS_CONV/COLS", "tiled:ROWS_CONV/COLS_CONV", "tiled:ROWS_CONV/ROWS_GEN"],
            ["tiled:ROWS_CAT/ROWS", "tiled:ROWS_CAT/COLS", "tiled:ROWS_CAT/COLS_CONV", "tiled:ROWS_CAT/ROWS_GEN"],
            _GEN4]
_GENERIC_AU = _GENERIC[:2] + [_GEN4, _GEN4, _GEN4]          # an unaligned conv / cat A is a ROWS_GEN
_SMALL_PLAIN = [["direct:ROWS/ROWS", "direct:ROWS/COLS", "tiled:ROWS/COLS_CONV", "tiled:ROWS/ROWS_GEN"],
                ["direct:COLS/ROWS", "direct:COLS/COLS", "tiled:COLS/COLS_CONV", "tiled:COLS/ROWS_GEN"]]
KIND_TABLE = {
    ("SMALL", None): [
        ["direct:ROWS/ROWS", "direct:ROWS/COLS", "tiled*:ROWS/COLS_CONV", "tiled:ROWS/ROWS_GEN"],
        ["direct:COLS/ROWS", "direct:COLS/COLS", "tiled*:COLS/COLS_CONV", "tiled:COLS/ROWS_GEN"],
        ["tiled*:ROWS_CONV/ROWS", "tiled*:ROWS_CONV/COLS", "tiled*:ROWS_CONV/COLS_CONV", "tiled:ROWS_CONV/ROWS_GEN"],
        ["direct:ROWS_CAT/ROWS", "direct:ROWS_CAT/COLS", "tiled*:ROWS_CAT/COLS_CONV", "tiled:ROWS_CAT/ROWS_GEN"],
        ["direct:ROWS_GEN/ROWS", "direct:ROWS_GEN/COLS", "tiled:ROWS_GEN/COLS_CONV", "tiled:ROWS_GEN/ROWS_GEN"]],
    ("SMALL", "a"): _SMALL_PLAIN + [_DGEN4, _DGEN4, _DGEN4],
    ("SMALL", "b"): _SMALL_PLAIN + [
        _GENERIC[2],
        ["direct:ROWS_CAT/ROWS", "direct:ROWS_CAT/COLS", "tiled:ROWS_CAT/COLS_CONV", "tiled:ROWS_CAT/ROWS_GEN"],
        _DGEN4],
    ("TILED", None): [
        ["tiled*:ROWS/ROWS", "tiled*:ROWS/COLS", "tiled*:ROWS/COLS_CONV", "tiled:ROWS/ROWS_GEN"],
        ["tiled*:COLS/ROWS", "tiled*:COLS/COLS", "tiled*:COLS/COLS_CONV", "tiled:COLS/ROWS_GEN"],
        ["tiled*:ROWS_CONV/ROWS", "tiled*:ROWS_CONV/COLS", "tiled*:ROWS_CONV/COLS_CONV", "tiled:ROWS_CONV/ROWS_GEN"],
        ["tiled*:ROWS_CAT/ROWS", "tiled*:ROWS_CAT/COLS", "tiled*:ROWS_CAT/COLS_CONV", "tiled:ROWS_CAT/ROWS_GEN"],
        _GEN4],
    ("TILED", "a"): _GENERIC_AU,
    ("TILED", "b"): _GENERIC,
    ("WIDE", None): [
        ["wide8:ROWS/ROWS", "wide8:ROWS/COLS", "wide8:ROWS/COLS_CONV", "tiled:ROWS/ROWS_GEN"],
        ["wide8:COLS/ROWS", "wide8:COLS/COLS", "wide8:COLS/COLS_CONV", "tiled:COLS/ROWS_GEN"],
        ["wide8:ROWS_CONV/ROWS", "wide8:ROWS_CONV/COLS", "wide8:ROWS_CONV/COLS_CONV", "tiled:ROWS_CONV/ROWS_GEN"],
        ["wide8:ROWS_CAT/ROWS", "wide8:ROWS_CAT/COLS", "wide8:ROWS_CAT/COLS_CONV", "tiled:ROWS_CAT/ROWS_GEN"],
        _GEN4],
    ("WIDE", "a"): _GENERIC_AU,
    ("WIDE", "b"): _GENERIC,
}


def _kind_desc(shape, aform, bform, unaligned):
    M, N = SHAPES[shape]
    K = 192 if aform == "conv" else 128          # a conv A has K = 3 cin (cin 64)
    if bform == "conv":
        N = N // 3 // 8 * 8 * 3                  # a conv B has N = 3 cin, cin % 8 == 0
    return fake_desc(M, N, K, a=aform + ("+u" if unaligned == "a" else ""),
                     b=bform + ("+u" if unaligned == "b" else ""))


@pytest.mark.parametrize("shape,unaligned", list(KIND_TABLE), ids=[f"{s}-{u or 'aligned'}" for s, u in KIND_TABLE])
def test_kind_table(lib, shape, unaligned):
    """Every A form x B form x alignment x shape class: the query answers FX_OK with a (family, A kind, B kind)
    that the family's pair predicate accepts -- a launch the dispatcher can instantiate -- or FX_ERR_UNSUPPORTED;
    the answers are pinned."""
    got = []
    for aform in A_FORMS:
        row = []
        for bform in B_FORMS:
            st, p = plan_of(_kind_desc(shape, aform, bform, unaligned))
            assert st in (0, ERR_UNSUPPORTED), (aform, bform, st, lib.fx_last_error())
            if st:
                row.append("unsupported")
                continue
            assert family_accepts(p), (aform, bform, gc.plan_dict(p))
            row.append(f"{gc.FAMILY_NAMES[p.family]}{'*' if p.fast else ''}:{KINDS[p.a_kind]}/{KINDS[p.b_kind]}")
        got.append(row)
    assert got == KIND_TABLE[(shape, unaligned)]


@pytest.mark.parametrize("prec", ["bf16", "fp32s", "fp32s2"])
def test_kind_table_under_precision_modes(prec):
    """The same forms under the precision modes: still a pair its family runs (the kinds do not depend on it)."""
    for shape in SHAPES:
        for aform in A_FORMS:
            for bform in B_FORMS:
                st, p = plan_of(_kind_desc(shape, aform, bform, None), prec)
                st0, p0 = plan_of(_kind_desc(shape, aform, bform, None))
                assert st == st0 == 0 and family_accepts(p), (shape, aform, bform)
                assert (p.a_kind, p.b_kind) == (p0.a_kind, p0.b_kind)


def test_refused_operands(lib):
    b = fake_operand("convB", 96, 128, gc.ADDR_B)
    b.trans = 0
    st, _ = plan_of(fake_desc(768, 96, 128, b=b))
    assert st == ERR_SHAPE and b"row-major conv B operand is not supported" in lib.fx_last_error()
    for side in ("a", "b"):
        o = fake_operand("rows", 768, 128, gc.ADDR_A)
        o.ones_col = 768
        st, _ = plan_of(fake_desc(768, 768, 128, **{side: o}))
        assert st == ERR_SHAPE and b"ones_col needs trans==1" in lib.fx_last_error()
    o = fake_operand("cols", 769, 128, gc.ADDR_B)            # with trans it plans: the fused bias column
    o.ones_col, o.ld = 769, 768
    assert plan(768, 769, 128, a="cols", b=o, c_last_col=gc.ADDR_POS).family == TILED
    a = fake_operand("convA", 768, 192, gc.ADDR_A)
    st, _ = plan_of(fake_desc(768, 768, 128, a=a))
    assert st == ERR_SHAPE and b"conv A needs K == taps*cin" in lib.fx_last_error()
