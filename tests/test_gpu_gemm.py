"""fx_gemm across its kernels (64x64 LDS-tiled / 128x64 wide / direct small-shape) and every epilogue option,
vs float64 torch on the same inputs (GPU).  Shapes are picked so the automatic path choice
exercises: direct (token rows, shallow K, few tiles, batched heads, cross-block split-K with the
fused last-block reduction) and tiled (with and without split-K, reduced in the launch and by the
reduce launch); every case asserts the path it names through the plan query fx_gemm_plan."""
import pytest
import torch

from factmx import functional as fxf
from factmx import native as nx
from gemm_cases import im2col

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _r(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


def _operand(t2d_or_3d, trans, batch_stride=0):
    o = nx.Operand()
    o.ptr = nx.ptr(t2d_or_3d)
    o.ld = t2d_or_3d.shape[-1]
    o.trans = int(trans)
    o.conv_dir = 1
    o.batch_stride = batch_stride
    return o


D, T, W = nx.GEMM_FAM_DIRECT, nx.GEMM_FAM_TILED, nx.GEMM_FAM_WIDE8
CASES = [
    # M, N, K, batch, a_trans, b_trans, split, the plan the label claims: (family, split taken, in-launch reduction),
    # asserted through fx_gemm_plan on the launched descriptor
    (32, 512, 512, 1, False, False, 1, (D, 1, 0)),      # token projection (direct)
    (32, 256, 1024, 1, False, True, 4, (D, 4, 1)),      # token dX (direct, split-K, last block reduces)
    (256, 257, 32, 1, True, True, 1, (D, 1, 0)),        # token dW, K = Nact (direct)
    (256, 257, 4096, 1, True, True, 13, (T, 13, 0)),    # frame-level dW, few tiles: K > 2048 keeps it tiled, reduce launch
    (4096, 32, 32, 8, True, True, 1, (D, 1, 0)),        # per-head attention products (direct, batched)
    (32, 32, 4096, 8, False, True, 32, (D, 16, 0)),     # per-head dK/dV-like (direct, batched, split 16: reduce launch)
    (96, 200, 1000, 1, False, False, 1, (D, 1, 0)),     # ragged edges (direct)
    (7, 5, 3, 1, False, True, 1, (D, 1, 0)),            # tiny
    (600, 520, 300, 1, False, False, 1, (D, 1, 0)),     # K <= 512 with a K tail: direct
    (800, 700, 320, 1, False, False, 1, (T, 1, 0)),     # tiled, FAST loaders
    (600, 520, 3000, 1, True, False, 6, (T, 6, 0)),     # tiled split-K, 6 slabs: reduce launch
    (600, 520, 3000, 1, True, False, 2, (T, 2, 1)),     # tiled split-K, 2 slabs: the last block of a tile reduces
    (1000, 700, 77, 2, False, True, 1, (D, 1, 0)),      # batched, ragged, shallow K tail: direct
    (1000, 700, 577, 2, False, True, 1, (T, 1, 0)),     # tiled, batched, ragged (K tail on the generic loop)
    (600, 520, 3001, 1, True, True, 6, (W, 6, 0)),      # weight gradient, K tail (COLS_KT: rows past K read as zero), wide tile
    (600, 520, 3001, 1, True, True, 3, (T, 3, 0)),      # the same on the 64 x 64 kernel's K-tail loaders
    (512, 513, 6996, 1, True, True, 13, (T, 13, 0)),    # the shipped yaml's ragged 4096 + 2900 rows (ld 513: generic loop)
    (640, 256, 1000, 2, True, True, 1, (D, 1, 0)),      # K tail, batched, few tiles: direct
]


@pytest.mark.parametrize("M,N,K,batch,at,bt,split,want", CASES, ids=["-".join(str(v) for v in c[:7]) for c in CASES])
@pytest.mark.parametrize("epi", ["plain", "bias_relu_resid", "beta_gate"])
def test_gemm(M, N, K, batch, at, bt, split, want, epi):
    A = _r(batch, M, K, seed=1)
    B = _r(batch, K, N, seed=2, scale=K ** -0.5)
    Ad = (A.transpose(1, 2) if at else A).contiguous().float().to(DEV)
    Bd = (B if bt else B.transpose(1, 2)).contiguous().float().to(DEV)
    a = _operand(Ad, at, Ad[0].numel())
    b = _operand(Bd, bt, Bd[0].numel())
    ref = A @ B
    c0 = _r(batch, M, N, seed=3)
    c = c0.float().to(DEV).contiguous()
    kw = {}
    if epi == "bias_relu_resid" and batch == 1:
        bias, resid = _r(N, seed=4), _r(M, N, seed=5)
        kw = dict(bias=bias.float().to(DEV), resid=resid.float().to(DEV), relu=1)
        ref = torch.relu(ref + bias + resid)
    elif epi == "beta_gate" and batch == 1:
        gate = _r(M, N, seed=6)
        kw = dict(beta=0.5, gate=gate.float().to(DEV))
        ref = torch.where(gate > 0, ref + 0.5 * c0, torch.zeros_like(ref))
    elif epi != "plain":
        pytest.skip("epilogue operands are single-batch")
    plan = nx.GemmPlanInfo()
    fxf.gemm(M, N, K, a, b, c, N, split=split, batch=batch, c_bs=M * N, plan=plan, **kw)
    torch.cuda.synchronize()
    assert (plan.family, plan.split, plan.in_launch_reduce) == want
    err = (c.double().cpu() - ref).abs().max().item()
    assert err <= 1e-5 * (1 + ref.abs().max().item()) + 1e-6 * K ** 0.5, err


@pytest.mark.parametrize("M,K,split", [(256, 32, 1), (256, 4096, 13), (512, 4096, 5), (512, 6996, 13), (256, 2900, 1)])
def test_gemm_fused_bias_column(M, K, split):
    """dW|db in one GEMM: the B operand's last column is a virtual ones column (c_last gets row sums)."""
    N1 = 200
    dy = _r(K, M, seed=7)         # (rows, out)
    x = _r(K, N1, seed=8)         # (rows, in)
    dyd, xd = dy.float().to(DEV), x.float().to(DEV)
    dw = _r(M, N1, seed=9)
    db = _r(M, seed=10)
    dwd, dbd = dw.float().to(DEV).contiguous(), db.float().to(DEV).contiguous()
    b = _operand(xd, True)
    b.ones_col = N1 + 1
    fxf.gemm(M, N1 + 1, K, _operand(dyd, True), b, dwd, N1, beta=1.0, split=split, c_last=dbd)
    torch.cuda.synchronize()
    # fp32 accumulation over K terms of unit-variance products: rounding grows ~sqrt(K) (the 128x64
    # tile runs one serial MFMA chain per split instead of two k-halves, so ~1.4x the 64x64 error).
    atol = max(1e-4, 5e-6 * K ** 0.5)
    torch.testing.assert_close(dwd.double().cpu(), dw + dy.t() @ x, rtol=1e-5, atol=atol)
    torch.testing.assert_close(dbd.double().cpu(), db + dy.sum(0), rtol=1e-5, atol=atol)


# ---------------------------------------------------------------- every (family, A kind, B kind) a plan can reach
# Operand forms (csrc/gemm_dev.h Kind): rows / cols = plain row- / column-major, conv = implicit 3-tap dilated
# conv (row-major A: ROWS_CONV, column-major B: COLS_CONV), cat = two sources side by side (ROWS_CAT), gen = rows
# plus a positional add (ROWS_GEN, the generic element fetch).  "+u" pads the leading dimension by one float, so
# the operand is not 16-B vector-loadable and the launch takes the generic loaders.
def _f32(*shape, seed, scale=1.0):
    return _r(*shape, seed=seed, scale=scale).float().double()   # float64 holding exactly the fp32 inputs


def _dev(X, unaligned):
    """fp32 device copy of a 2-d float64 matrix, its leading dimension one float longer when `unaligned`."""
    buf = torch.zeros(X.shape[0], X.shape[1] + int(unaligned), device=DEV)
    buf[:, :X.shape[1]] = X.float().to(DEV)
    return buf


def _make(form, R, K, seed):
    """Operand of R rows over K in the given form: (fx_operand, its (R, K) float64 value, tensors to keep)."""
    kind, _, flag = form.partition("+")
    u = flag == "u"
    o = nx.Operand()
    o.conv_dir = 1
    if kind in ("rows", "gen"):
        X = _f32(R, K, seed=seed)
        keep = [_dev(X, u)]
        o.ptr, o.ld = nx.ptr(keep[0]), keep[0].shape[1]
        if kind == "gen":
            pc = min(K, 40)
            pos = _f32(R, pc, seed=seed + 50)
            keep.append(pos.float().to(DEV).contiguous())
            o.pos, o.ld_pos, o.pos_cols = nx.ptr(keep[1]), pc, pc
            X = X.clone()
            X[:, :pc] += pos
        return o, X, keep
    if kind == "cols":
        X = _f32(R, K, seed=seed)
        keep = [_dev(X.t().contiguous(), u)]
        o.ptr, o.ld, o.trans = nx.ptr(keep[0]), keep[0].shape[1], 1
        return o, X, keep
    if kind == "cat":
        ks = 64
        X = _f32(R, K, seed=seed)
        keep = [_dev(X[:, :ks].contiguous(), u), _dev(X[:, ks:].contiguous(), u)]
        o.ptr, o.ld, o.ptr1, o.ld1, o.k_split = nx.ptr(keep[0]), keep[0].shape[1], nx.ptr(keep[1]), keep[1].shape[1], ks
        return o, X, keep
    raise AssertionError(form)


def _make_conv(R, cin, seq_len, dil, trans, u, seed):
    X = _f32(R, cin, seed=seed)
    keep = [_dev(X, u)]
    o = nx.Operand()
    o.ptr, o.ld, o.trans, o.conv_dir = nx.ptr(keep[0]), keep[0].shape[1], int(trans), 1
    o.conv_taps, o.conv_cin, o.conv_dil, o.seq_len = 3, cin, dil, seq_len
    return o, im2col(X, dil, seq_len), keep


# shapes by family, from the planner's thresholds: wide8 from 192 tiles of 128 x 64 with K % 64 == 0; below that
# and past 512 tiles of 32 x 32 the 64 x 64 tiled kernel; token rows (M = 32) the direct kernel.  A conv A has
# K = 3 cin (cin 64), a conv B has N = 3 cin.
WIDE, TILED, SMALL = (1536, 1024), (768, 768), (32, 96)
PAIR_CASES = (
    # the 128 x 64 f32 kernel
    [("wide8", a, b, WIDE, "fp32") for a, b in [("rows", "conv"), ("conv", "cols"), ("conv", "conv"), ("cat", "cols"),
                                                 ("cat", "conv"), ("cols", "rows")]]
    # the precision modes on the same tile: bf16 kernel, split kernel (B cols) / register split (B rows)
    + [("prec", a, b, WIDE, p) for p in ("bf16", "fp32s", "fp32s2") for a in ("rows", "conv", "cat")
       for b in ("rows", "cols")]
    # the 64 x 64 kernel, FAST loaders
    + [("tiled", a, b, TILED, "fp32") for a, b in [("rows", "conv"), ("conv", "cols"), ("conv", "conv"),
                                                   ("cat", "cols"), ("cat", "conv"), ("cols", "rows")]]
    # the 64 x 64 kernel, generic loaders: B not vector-loadable, or a positional add on either side
    + [("generic", a, b, TILED, "fp32") for a in ("rows", "conv", "gen", "cols", "cat")
       for b in ("rows+u", "cols+u", "conv+u", "gen")]
    # the direct kernel's pairs the model's shapes leave out
    + [("direct", a, b, SMALL, "fp32") for a, b in [("gen", "cols"), ("cat", "cols"), ("cols", "rows")]]
)


@pytest.mark.parametrize("family,aform,bform,MN,prec", PAIR_CASES,
                         ids=[f"{f}-{a}-{b}-{p}" for f, a, b, _, p in PAIR_CASES])
def test_gemm_family_pairs(family, aform, bform, MN, prec):
    """One launch per (kernel family, A kind, B kind) that the planner can reach and the model's own shapes
    in this suite do not, at the smallest shape that selects the family, against float64 torch.  fp32 and
    the 3-piece split keep the file's fp32 tolerance; bf16 rounds both operands to 8 significant bits
    (each within 2^-9, so a product within 2^-8) and the 2-piece split keeps 16 (~2^-16 per product): those
    two add that fraction of |A| |B|, the bound of the number format."""
    M, N = MN
    K = 192 if aform.startswith("conv") else 128
    if bform.startswith("conv"):
        N = N // 3 // 8 * 8 * 3   # 3 taps of cin channels, cin % 8 == 0 (1008 still gives the wide kernel 192 tiles)
    if aform.startswith("conv"):
        a, A, ka = _make_conv(M, 64, 256, 3, False, aform.endswith("+u"), seed=21)
    else:
        a, A, ka = _make(aform, M, K, seed=21)
    if bform.startswith("conv"):
        b, Bt, kb = _make_conv(K, N // 3, 64, 2, True, bform.endswith("+u"), seed=22)   # (K, N) value
    else:
        b, Bn, kb = _make(bform, N, K, seed=22)
        Bt = Bn.t()
    ref = A @ Bt
    c = torch.empty(M, N, device=DEV)
    plan = nx.GemmPlanInfo()
    with fxf.gemm_precision(prec):
        fxf.gemm(M, N, K, a, b, c, N, plan=plan)
    torch.cuda.synchronize()
    want = {"wide8": nx.GEMM_FAM_WIDE8, "tiled": nx.GEMM_FAM_TILED, "generic": nx.GEMM_FAM_TILED,
            "direct": nx.GEMM_FAM_DIRECT}.get(family)
    if family == "prec":   # the bf16 kernel; the split modes: the split kernel (B cols) / register split (B rows)
        want = (nx.GEMM_FAM_BF16 if prec == "bf16" else
                nx.GEMM_FAM_SPLIT if bform == "cols" else nx.GEMM_FAM_WIDE8)
        assert plan.np == {"bf16": 0, "fp32s": 3, "fp32s2": 2}[prec]
    assert plan.family == want and plan.fast == int(family == "tiled"), (plan.family, plan.fast)
    err = (c.double().cpu() - ref).abs()
    tol = 1e-5 * (1 + ref.abs().max().item()) + 1e-6 * K ** 0.5
    print(f"{family} {aform} x {bform} {prec}: max err {err.max().item():.3e} (fp32 tolerance {tol:.3e})")
    if prec in ("bf16", "fp32s2"):
        bound = ((1 + 2.0 ** -9) ** 2 - 1 if prec == "bf16" else 2.0 ** -16) * (A.abs() @ Bt.abs()) + tol
        assert bool((err <= bound).all()), (err - bound).max().item()
    else:
        assert err.max().item() <= tol, err.max().item()


def test_split_k_repeat_is_deterministic():
    """The per-tile arrival counters re-arm: back-to-back split-K launches give identical bits."""
    A = _r(3000, 64, seed=11).float().to(DEV)
    B = _r(3000, 96, seed=12).float().to(DEV)
    outs = []
    for _ in range(3):
        c = torch.empty(64, 96, device=DEV)
        fxf.gemm(64, 96, 3000, _operand(A, True), _operand(B, True), c, 96, split=8)
        outs.append(c)
    for _ in range(3):
        c = torch.empty(64, 96, device=DEV)
        fxf.gemm(64, 96, 3000, _operand(A, True), _operand(B, True), c, 96, split=3)
        outs.append(c)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[1], outs[2])
    assert torch.equal(outs[3], outs[4])
    torch.testing.assert_close(outs[0], outs[3], rtol=1e-5, atol=1e-4)
