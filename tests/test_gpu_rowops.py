"""Launch-geometry edges of the row-wise kernels (csrc/rowops.hip) against float64 torch on the CPU (GPU).

LayerNorm, process_feature, L2 normalise and dropout are called through the C entry points (ctypes) wherever a
leading dimension, a null pointer or an accumulate-into buffer has to be controlled, through
factmx.functional otherwise.  Every reference is fed the exact fp32 input values (``.float().double()``).
Strided operands (ld = cols + 3): the padding of an input holds NaN (a read past ``cols`` poisons the
result), the padding of an output holds a sentinel that must be unchanged afterwards.
Bounds are those of tests/test_gpu_kernels.py (test_layernorm_fused_residual_relu,
test_process_feature_and_l2norm): forward values 2e-5 + 2e-5 max|ref|, LayerNorm gradients 1e-4 + 1e-4 max|ref|."""
import numpy as np
import pytest
import torch

from helpers import drop_mask
from factmx import functional as fxf
from factmx import native as nx
from oracle import fact_oracle as fo

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 3
SENTINEL = -777.25


def _r(*shape, seed, scale=1.0):
    """float64 tensor holding exact fp32 values."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale).float().double()


def _close(a, b, rtol=2e-5, atol=2e-5, what=""):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert torch.isfinite(a).all(), f"{what}: non-finite values"
    err = (a - b).abs().max().item() if a.numel() else 0.0
    ref = b.abs().max().item() if b.numel() else 0.0
    assert err <= atol + rtol * ref, f"{what}: max err {err:.3e} (ref max {ref:.3e})"


class _Buf:
    """A (rows, cols) device operand inside a (rows, cols + pad) buffer whose padding holds ``fill``."""

    def __init__(self, rows, cols, pad, fill, value=None):
        self.rows, self.cols, self.pad, self.fill = rows, cols, pad, fill
        self.full = torch.full((rows, cols + pad), float(fill), device=DEV)
        if value is not None:
            self.full[:, :cols] = value.float().to(DEV)

    @property
    def ptr(self):
        return self.full.data_ptr()

    @property
    def ld(self):
        return self.cols + self.pad

    def view(self):
        return self.full[:, :self.cols]

    def check_padding(self, what):
        if self.pad:
            padv = self.full[:, self.cols:]
            assert torch.equal(padv, torch.full_like(padv, float(self.fill))), f"{what}: padding overwritten"


def _inp(t, pad):
    return _Buf(t.shape[0], t.shape[1], pad, float("nan"), t)


def _out(rows, cols, pad):
    return _Buf(rows, cols, pad, SENTINEL)


def _guarded(v, fill):
    """A device vector of len(v) + 1 floats: v, then one guard element holding ``fill``."""
    t = torch.full((v.numel() + 1,), float(fill), device=DEV)
    t[:-1] = v.float().to(DEV)
    return t


# ---------------------------------------------------------------- LayerNorm
# (rows, cols): the constant or branch of rowops.hip the shape reaches.  The backward takes the one-block
# ln_bwd_small_kernel for rows <= 16 * SMALL_RPW = 64 and cols <= 64 * SMALL_CPL = 256, else ln_bwd_kernel on
# min(ceil(rows / 4), LN_BWD_MAXBLK) row blocks + ln_bwd_reduce (8 interleaved groups of row blocks).
LN_SHAPES = [
    (1, 1),        # smallest shape: one lane of one wave active; variance 0, rstd = eps^-1/2 (small backward)
    (3, 48),       # cols below one 64-lane chunk; 3 of the 16 waves of the small backward own a row
    (64, 256),     # last shape on the small backward: rows = 16 * SMALL_RPW and cols = 64 * SMALL_CPL
    (65, 256),     # first row count off it (rows > 16 * SMALL_RPW): general backward, 17 row blocks
    (64, 257),     # first col count off it (cols > 64 * SMALL_CPL): general backward, 16 row blocks
    (5, 320),      # general backward with 2 row blocks: 6 of ln_bwd_reduce's 8 partial groups own nothing
    (37, 75),      # ragged cols (75 = 64 + 11) and rows (37 = 2 * 16 + 5) on the small backward
    (30, 1024),    # the cols limit 64 * MAXPL: every one of the 16 register slots per lane in use
    (4101, 96),    # rows > 4 * LN_BWD_MAXBLK = 4096: blocks 0 and 1 of the 1024 take a second pass of the
                   # grid-stride row loop, block 1's (rows 4100..4103) partial
]


def _ln_case(rows, cols, residual, relu, pad=0, grads="acc", seed=0):
    """fx_layernorm_fwd + fx_layernorm_bwd at one shape and form; grads: "acc" (dw / db pre-filled with random
    values: the result is old + gradient), "no_dw", "no_db", "none" (both null, and a null workspace)."""
    lib = nx.load()
    x, r = _r(rows, cols, seed=seed + 1), _r(rows, cols, seed=seed + 2)
    w, b = (1 + 0.1 * _r(cols, seed=seed + 3)).float().double(), _r(cols, seed=seed + 4, scale=0.1)
    dy = _r(rows, cols, seed=seed + 5)
    dw0, db0 = _r(cols, seed=seed + 6), _r(cols, seed=seed + 7)
    xb, rb, dyb = _inp(x, pad), (_inp(r, pad) if residual else None), _inp(dy, pad)
    yb, xhb, dxb = _out(rows, cols, pad), _out(rows, cols, pad), _out(rows, cols, pad)
    # the vectors carry one guard element past cols: NaN behind w / b, the sentinel behind dw / db
    wd, bd = _guarded(w, float("nan")), _guarded(b, float("nan"))
    rstd = torch.full((rows + 1,), SENTINEL, device=DEV)
    st = lib.fx_layernorm_fwd(xb.ptr, xb.ld, rb.ptr if rb else None, rb.ld if rb else 0, nx.ptr(wd), nx.ptr(bd), 1e-5,
                              rows, cols, int(relu), yb.ptr, yb.ld, xhb.ptr, xhb.ld, nx.ptr(rstd), nx.stream())
    nx.check(st, "fx_layernorm_fwd")
    dw = None if grads in ("no_dw", "none") else _guarded(dw0, SENTINEL)
    db = None if grads in ("no_db", "none") else _guarded(db0, SENTINEL)
    nws = lib.fx_layernorm_bwd_workspace_floats(rows, cols)
    ws = None if grads == "none" else torch.empty(max(nws, 1), device=DEV)
    st = lib.fx_layernorm_bwd(dyb.ptr, dyb.ld, yb.ptr, yb.ld, xhb.ptr, xhb.ld, nx.ptr(wd), nx.ptr(rstd), rows, cols,
                              int(relu), dxb.ptr, dxb.ld, nx.ptr(dw), nx.ptr(db), nx.ptr(ws), nx.stream())
    nx.check(st, "fx_layernorm_bwd")
    torch.cuda.synchronize()
    # float64 reference; with relu the backward gate is the GPU's own y > 0 (a pre-activation within fp32
    # noise of 0 may land on either side), so no element is left out of any comparison
    y_gpu = yb.view().double().cpu()
    vr = (x + r if residual else x.clone()).requires_grad_(True)
    wr, br = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    yr = fo.layer_norm(vr, wr, br)
    if relu:
        yr = yr * (y_gpu > 0).double()
        if rows * cols >= 48:
            assert (y_gpu > 0).any() and (y_gpu == 0).any(), "relu case needs both signs"
    (yr * dy).sum().backward()
    mu = vr.detach().mean(-1, keepdim=True)
    rs_ref = 1.0 / torch.sqrt(((vr.detach() - mu) ** 2).mean(-1) + 1e-5)
    _close(y_gpu, yr, what="y")
    _close(xhb.view(), (vr.detach() - mu) * rs_ref[:, None], what="xhat")
    _close(rstd[:rows], rs_ref, what="rstd")
    assert rstd[rows].item() == SENTINEL, "rstd written past rows"
    _close(dxb.view(), vr.grad, rtol=1e-4, atol=1e-4, what="dx")
    if dw is not None:
        _close(dw[:cols], dw0 + wr.grad, rtol=1e-4, atol=1e-4, what="dw (old + gradient)")
        assert dw[cols].item() == SENTINEL, "dw written past cols"
    if db is not None:
        _close(db[:cols], db0 + br.grad, rtol=1e-4, atol=1e-4, what="db (old + gradient)")
        assert db[cols].item() == SENTINEL, "db written past cols"
    for buf, name in ((yb, "y"), (xhb, "xhat"), (dxb, "dx")):
        buf.check_padding(name)


@pytest.mark.parametrize("residual,relu", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("rows,cols", LN_SHAPES)
def test_layernorm_shapes(rows, cols, residual, relu):
    _ln_case(rows, cols, residual, relu, seed=10 * rows + cols)


# one shape per backward kernel: (37, 75) ln_bwd_small_kernel, (5, 320) and (65, 256) ln_bwd_kernel + ln_bwd_reduce
@pytest.mark.parametrize("rows,cols", [(37, 75), (5, 320), (65, 256)])
def test_layernorm_leading_dimensions(rows, cols):
    """x, r, y, xhat, dy and dx all with ld = cols + 3: NaN in the inputs' padding, a sentinel in the outputs'."""
    _ln_case(rows, cols, True, True, pad=PAD, seed=7)
    _ln_case(rows, cols, False, False, pad=PAD, seed=8)


# (3, 48): ln_bwd_small_kernel accumulates in its own launch (no workspace at all); (5, 320): ln_bwd_kernel gets a
# null workspace when neither gradient is wanted and ln_bwd_reduce is not launched; (4101, 96): the same with the
# grid-stride loop
@pytest.mark.parametrize("grads", ["no_dw", "no_db", "none"])
@pytest.mark.parametrize("rows,cols", [(3, 48), (5, 320), (4101, 96)])
def test_layernorm_null_gradients(rows, cols, grads):
    _ln_case(rows, cols, True, False, grads=grads, seed=9)


def test_layernorm_bwd_refuses_null_workspace_with_gradients():
    """dw wanted off the one-block backward, workspace null: an error status, nothing launched."""
    lib = nx.load()
    src = torch.ones(65 * 256, device=DEV)
    dx, dw = torch.full((65 * 256,), SENTINEL, device=DEV), torch.full((256,), SENTINEL, device=DEV)
    st = lib.fx_layernorm_bwd(nx.ptr(src), 256, nx.ptr(src), 256, nx.ptr(src), 256, nx.ptr(src), nx.ptr(src), 65, 256,
                              0, nx.ptr(dx), 256, nx.ptr(dw), None, None, nx.stream())
    assert st != 0 and b"workspace" in lib.fx_last_error()
    torch.cuda.synchronize()
    assert torch.equal(dx, torch.full_like(dx, SENTINEL)) and torch.equal(dw, torch.full_like(dw, SENTINEL))


@pytest.mark.parametrize("cols", [1025, 0])   # past 64 * MAXPL, and the empty row
def test_layernorm_refuses_cols_out_of_range(cols):
    """An error status, and nothing launched: every output buffer keeps its sentinel."""
    lib = nx.load()
    rows, n = 4, 4 * 1025
    src = torch.ones(n, device=DEV)
    outs = [torch.full((n,), SENTINEL, device=DEV) for _ in range(6)]
    y, xhat, rstd, dx, dw, db = outs
    ws = torch.full((lib.fx_layernorm_bwd_workspace_floats(rows, 1025),), SENTINEL, device=DEV)
    st = lib.fx_layernorm_fwd(nx.ptr(src), 1025, nx.ptr(src), 1025, nx.ptr(src), nx.ptr(src), 1e-5, rows, cols, 0,
                              nx.ptr(y), 1025, nx.ptr(xhat), 1025, nx.ptr(rstd), nx.stream())
    assert st != 0 and b"cols" in lib.fx_last_error()
    st = lib.fx_layernorm_bwd(nx.ptr(src), 1025, nx.ptr(src), 1025, nx.ptr(src), 1025, nx.ptr(src), nx.ptr(src), rows,
                              cols, 0, nx.ptr(dx), 1025, nx.ptr(dw), nx.ptr(db), nx.ptr(ws), nx.stream())
    assert st != 0 and b"cols" in lib.fx_last_error()
    torch.cuda.synchronize()
    for t in outs + [ws]:
        assert torch.equal(t, torch.full_like(t, SENTINEL))


# ---------------------------------------------------------------- process_feature
# (rows, cols, n): one wave per row, lanes striding the n class columns and the cols - n feature columns by 64
PF_CASES = [
    (1, 1, 1),         # smallest: no feature column, a softmax over one class (probability 1, gradient 0)
    (5, 40, 1),        # n = 1 beside 39 feature columns; rows 4..7 of the second 4-row block do not exist
    (6, 33, 33),       # n = cols: no feature column at all (f = 0)
    (9, 100, 17),      # n < 64: 47 lanes idle in both wave reductions; f = 83 takes two passes of the copy loop
    (130, 700, 201),   # n = 3 * 64 + 9 and f = 7 * 64 + 51: partial last passes; 33 row blocks, the last partial
]


def _pf_case(rows, cols, n, with_clogit, pad=0):
    lib = nx.load()
    x = _r(rows, cols, seed=21)
    g, gc = _r(rows, cols, seed=22), _r(rows, n, seed=23)
    xb, gb = _inp(x, pad), _inp(g, pad)
    ob, dxb = _out(rows, cols, pad), _out(rows, cols, pad)
    cb = _out(rows, n, pad) if with_clogit else None
    gcb = _inp(gc, pad) if with_clogit else None
    nx.check(lib.fx_process_feature_fwd(xb.ptr, xb.ld, rows, cols, n, ob.ptr, ob.ld, cb.ptr if cb else None,
                                        cb.ld if cb else 0, nx.stream()), "fx_process_feature_fwd")
    nx.check(lib.fx_process_feature_bwd(ob.ptr, ob.ld, gb.ptr, gb.ld, gcb.ptr if gcb else None, gcb.ld if gcb else 0,
                                        rows, cols, n, dxb.ptr, dxb.ld, nx.stream()), "fx_process_feature_bwd")
    torch.cuda.synchronize()
    xr = x.clone().requires_grad_(True)
    outr, clr = fo.process_feature(xr, n)
    loss = (outr * g).sum()
    if with_clogit:
        loss = loss + (clr * gc).sum()
    loss.backward()
    _close(ob.view(), outr, what="pf out")
    _close(dxb.view(), xr.grad, what="pf dx")
    ob.check_padding("out")
    dxb.check_padding("dx")
    if with_clogit:
        assert torch.equal(cb.view().cpu(), x[:, cols - n:].float()), "clogit is a copy of the class columns"
        cb.check_padding("clogit")


@pytest.mark.parametrize("with_clogit", [True, False])
@pytest.mark.parametrize("rows,cols,n", PF_CASES)
def test_process_feature_shapes(rows, cols, n, with_clogit):
    _pf_case(rows, cols, n, with_clogit)


def test_process_feature_leading_dimensions():
    """x, out, clogit, dout, dclogit and dx with ld = cols + 3 (clogit / dclogit: n + 3), poisoned padding."""
    _pf_case(9, 100, 17, True, pad=PAD)
    _pf_case(130, 700, 201, False, pad=PAD)


def test_process_feature_refuses_bad_n():
    lib = nx.load()
    out = torch.full((4 * 8,), SENTINEL, device=DEV)
    for n in (0, 9):
        st = lib.fx_process_feature_fwd(nx.ptr(out), 8, 4, 8, n, nx.ptr(out), 8, None, 0, nx.stream())
        assert st != 0 and b"process_feature" in lib.fx_last_error()
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full_like(out, SENTINEL))


# ---------------------------------------------------------------- L2 normalise
# 7 x 3: cols below the wave width, 2 row blocks; 66 x 130: three passes of the 64-lane column loop (the last with
# 2 lanes), 17 row blocks with the last one half filled
@pytest.mark.parametrize("rows,cols", [(7, 3), (66, 130)])
def test_l2_normalize_clamped_rows(rows, cols):
    """One row exactly zero and one row of 1e-20 (its sum of squares underflows in fp32): both norms are
    <= 1e-12, the row is clamped, y = x / eps and dx = dy / eps (about 1e12 dy).  Those rows are compared row by
    row relative to their own reference maximum -- inside one comparison they would swallow every other row's
    tolerance -- and the remaining rows as test_process_feature_and_l2norm does."""
    x = _r(rows, cols, seed=31)
    x[1] = 0.0
    x[rows - 2] = float(np.float32(1e-20))
    g = _r(rows, cols, seed=32)
    clamped = [1, rows - 2]
    rest = [i for i in range(rows) if i not in clamped]
    xd = x.float().to(DEV).requires_grad_(True)
    y = fxf.l2_normalize(xd)
    (y * g.float().to(DEV)).sum().backward()
    torch.cuda.synchronize()
    xr = x.clone().requires_grad_(True)
    yr = xr / xr.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    (yr * g).sum().backward()
    assert (xr.detach().norm(dim=-1)[clamped] <= 1e-12).all()
    _close(y[rest], yr[rest], what="l2n y")
    _close(xd.grad[rest], xr.grad[rest], what="l2n dx")
    for i in clamped:
        assert xr.grad[i].abs().max().item() > 1e9, "the clamped row's gradient is dy / eps"
        _close(y[i], yr[i], atol=0.0, what=f"l2n y, clamped row {i}")
        _close(xd.grad[i], xr.grad[i], atol=0.0, what=f"l2n dx, clamped row {i}")


def test_l2_normalize_leading_dimensions():
    lib = nx.load()
    rows, cols = 66, 130
    x, g = _r(rows, cols, seed=33), _r(rows, cols, seed=34)
    xb, gb = _inp(x, PAD), _inp(g, PAD)
    yb, dxb = _out(rows, cols, PAD), _out(rows, cols, PAD)
    nrm = torch.full((rows + 1,), SENTINEL, device=DEV)
    nx.check(lib.fx_l2norm_fwd(xb.ptr, xb.ld, rows, cols, yb.ptr, yb.ld, nx.ptr(nrm), nx.stream()), "fx_l2norm_fwd")
    nx.check(lib.fx_l2norm_bwd(yb.ptr, yb.ld, nx.ptr(nrm), gb.ptr, gb.ld, rows, cols, dxb.ptr, dxb.ld, nx.stream()),
             "fx_l2norm_bwd")
    torch.cuda.synchronize()
    xr = x.clone().requires_grad_(True)
    yr = xr / xr.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    (yr * g).sum().backward()
    _close(yb.view(), yr, what="l2n y")
    _close(nrm[:rows], xr.detach().norm(dim=-1), what="l2n norm")
    assert nrm[rows].item() == SENTINEL
    _close(dxb.view(), xr.grad, what="l2n dx")
    yb.check_padding("y")
    dxb.check_padding("dx")


# ---------------------------------------------------------------- dropout
def _dropout_case(rows, cols, p, seed, idx_ld=None, idx_col0=0, padx=0, pady=0, inplace=False):
    """fx_dropout against tests/helpers.drop_mask at the documented index r * idx_ld + idx_col0 + c; kept values
    are x / (1 - p) in fp32 and must match bitwise, dropped ones are +0."""
    lib = nx.load()
    idx_ld = cols if idx_ld is None else idx_ld
    x = _r(rows, cols, seed=41).float()
    xb = _inp(x, padx)
    yb = xb if inplace else _out(rows, cols, pady)
    nx.check(lib.fx_dropout(xb.ptr, xb.ld, rows, cols, idx_ld, idx_col0, float(p), seed, yb.ptr, yb.ld, nx.stream()),
             "fx_dropout")
    torch.cuda.synchronize()
    idx = np.arange(rows, dtype=np.int64)[:, None] * idx_ld + idx_col0 + np.arange(cols, dtype=np.int64)[None, :]
    keep = torch.from_numpy(drop_mask(seed, idx, p))
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    expect = torch.where(keep, x * scale, torch.zeros(()))
    assert 0 < keep.sum().item() < keep.numel()
    got = yb.view().cpu()
    assert torch.equal(got, expect), f"{(got != expect).sum().item()} of {got.numel()} elements differ"
    if inplace:
        padv = xb.full[:, cols:]
        assert torch.isnan(padv).all(), "in-place dropout wrote into the padding"
    else:
        yb.check_padding("y")


def test_dropout_grid_stride():
    """2100 x 512 = 1 075 200 elements > 4096 blocks x 256 threads: the first 26 624 threads take a second
    element (the block cap of launch_dropout)."""
    _dropout_case(2100, 512, 0.3, 0x1234567890ABCDEF)


def test_dropout_index_window():
    """A (5, 7) window at column 123 of a 1000-wide index space: idx_ld != cols and idx_col0 != 0."""
    _dropout_case(5, 7, 0.5, 0x0FEDCBA987654321, idx_ld=1000, idx_col0=123)


def test_dropout_leading_dimensions():
    """ldx = cols + 3 and ldy = cols + 5, both different from idx_ld = cols."""
    _dropout_case(33, 70, 0.2, 77, padx=3, pady=5)


def test_dropout_in_place():
    """y aliasing x (documented), in a buffer wider than cols and with an index window."""
    _dropout_case(300, 129, 0.5, 2 ** 63 + 5, idx_ld=200, idx_col0=17, padx=3, inplace=True)
