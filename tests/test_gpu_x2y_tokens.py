"""The X2Y attention cores at 65 .. 320 action tokens per video (the wide variants in x2y_a2f.hip and
x2y_f2a.hip) on the GPU against the fp64 oracle, through check_x2y of test_gpu_x2y.py and its tolerances (1e-4 on out, logit,
dX, dY and the positions, 1e-5 on attn, 2e-4 on the weights, each relative to 1 + max|ref|):

* a2f (keys = tokens): one key in a third 32-key block (65), a block edge and one past it (96, 97), 200, 300
  and the cap 320, over one partial 32-row workgroup, two ragged videos and a single query row -- calls of
  fewer than 1024 rows, which the dispatch keeps on the grouped GEMMs (the wide cores measured slower
  there, profiles/x2y_tokens.json) -- and over 1030 rows and two ragged videos of 700 + 413, which take the
  wide core; 321 keys once, which must still be right through the grouped GEMMs;
* f2a (queries = tokens): one query in a second 64-query block (65), a block edge and one past it (128,
  129), 300 and the cap 320, at segment-like key counts (below 1024 rows: the grouped GEMMs), a one-key
  video (the <= 64-key a2f core), 47 key chunks, 4097 keys and two ragged videos of 700 + 413 keys; every f2a case again in child
  processes with the fused backward forced (FX_X2Y_F2A_BWD=1: the wide f2a backward measured slower than
  the grouped GEMMs and is not the default at any size), as one launch with its grid barrier and as two;
* one call whose videos have 40 and 75 tokens, both directions;
* fx_prof counts prove which core ran; two runs are bitwise equal; the device status word stays clean.
"""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
for _p in (_ROOT, os.path.join(_ROOT, "fact-clip_amd"), _HERE):     # (the child process has no conftest)
    if _p not in sys.path:
        sys.path.insert(0, _p)
from factmx import functional as fxf  # noqa: E402
from factmx import native as nx  # noqa: E402
from oracle import fact_oracle as fo  # noqa: E402
import test_gpu_x2y as base  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
A, D2 = base.A, base.D2

A2F_KEYS = (65, 96, 97, 200, 300, 320)
A2F_FRAMES = ((33,), (300, 200), (1,), (1030,), (700, 413))
F2A_QUERIES = (65, 128, 129, 300, 320)
F2A_FRAMES = ((200, 90), (64, 1), (3000,))
# ((200, 90) keys: the grouped GEMMs, as every call below 1024 rows; (64, 1): the <= 64-key a2f core with up
# to 320 query rows; two ragged videos of 1113 keys are added for the wide f2a core)
F2A_CASES = ([(nq, Ts) for nq in F2A_QUERIES for Ts in F2A_FRAMES] + [(129, (4097,))] +
             [(nq, (700, 413)) for nq in (65, 320)])


def _checked(direction, nq, Ts):
    base.check_x2y(direction, nq, Ts)
    fxf.check_device_status()


@pytest.mark.parametrize("Ts", A2F_FRAMES)
@pytest.mark.parametrize("nk", A2F_KEYS)
def test_wide_a2f_vs_oracle(nk, Ts):
    _checked("a2f", nk, Ts)


def test_a2f_past_the_cap_takes_the_grouped_path():
    lib = nx.load()
    # (321 query rows too: with <= 320 of them the call would be the wide f2a core's)
    assert lib.fx_x2y_core(base.H, 1, None, None, 321, 321) == 0
    _checked("a2f", 321, (321,))


@pytest.mark.parametrize("nq,Ts", F2A_CASES)
def test_wide_f2a_vs_oracle(nq, Ts):
    _checked("f2a", nq, Ts)


@pytest.mark.parametrize("one_launch", ["1", "0"])
def test_wide_f2a_fused_backward_vs_oracle(one_launch):
    """The f2a cases again with the fused f2a backward core switched on for every call (by default the
    <= 64-query one runs from 64 key chunks and the wide one never), as one launch with a grid barrier
    between the dP and dlogit passes and as two launches (FX_X2Y_F2A_ONE=0); the child also counts the
    backward core's fx_prof bracket and compares two runs bitwise.  Child processes: the knobs are read
    when the library loads."""
    env = dict(os.environ, FX_X2Y_F2A_BWD="1", FX_X2Y_F2A_ONE=one_launch)
    p = subprocess.run([sys.executable, "-u", os.path.abspath(__file__), "f2a"], env=env, cwd=_ROOT, timeout=240)
    assert p.returncode == 0, p.returncode


def _run_x2y(direction, nqs, Ts, oracle):
    """check_x2y with a token count PER VIDEO (nqs): the outputs and every gradient, compared with the
    fp64 oracle under check_x2y's tolerances when `oracle`."""
    g = torch.Generator().manual_seed(7)
    nv = len(Ts)
    tok = [torch.randn(n, A, generator=g, dtype=torch.float64).float().double() for n in nqs]
    frm = [torch.randn(T, D2, generator=g, dtype=torch.float64).float().double() for T in Ts]
    tpos = [0.5 * torch.randn(n, A, generator=g, dtype=torch.float64).float().double() for n in nqs]
    fpos = [0.5 * torch.randn(T, D2, generator=g, dtype=torch.float64).float().double() for T in Ts]
    if direction == "a2f":           # X = tokens, Y = frames
        Xs, Ys, Xps, Yps, xdim, ydim = tok, frm, tpos, fpos, A, D2
    else:
        Xs, Ys, Xps, Yps, xdim, ydim = frm, tok, fpos, tpos, D2, A
    P = base._params(xdim, ydim, 192, seed=3)
    xl, yl = [0], [0]
    for X, Y in zip(Xs, Ys):
        xl.append(xl[-1] + X.shape[0])
        yl.append(yl[-1] + Y.shape[0])
    cat = lambda ts: torch.cat(ts).float().to(DEV).requires_grad_(True)   # noqa: E731
    X, Y, Xp, Yp = cat(Xs), cat(Ys), cat(Xps), cat(Yps)
    W = {n: t.float().to(DEV).requires_grad_(True) for n, t in P.items()}
    rows = (xl, yl) if nv > 1 else None
    out, logit, attn = base._X2YAttnGrad.apply(X, Y, Xp, Yp, rows, W["X_K.weight"], W["X_K.bias"], W["X_V.weight"],
                                               W["X_V.bias"], W["Y_Q.weight"], W["Y_Q.bias"], W["Y_W.weight"],
                                               W["Y_W.bias"], 0.0, 0)
    gen = torch.Generator().manual_seed(9)
    gout = torch.randn(out.shape, generator=gen, dtype=torch.float64)
    glog = torch.randn(logit.shape, generator=gen, dtype=torch.float64)
    gatt = torch.randn(attn.shape, generator=gen, dtype=torch.float64)
    loss = ((out.double() * gout.to(DEV)).sum() + (logit.double() * glog.to(DEV)).sum() +
            (attn.double() * gatt.to(DEV)).sum())
    loss.backward()
    torch.cuda.synchronize()
    got = {"out": out, "logit": logit, "attn": attn, "dX": X.grad, "dY": Y.grad, "dXpos": Xp.grad, "dYpos": Yp.grad}
    got.update({n: W[n].grad for n in P})
    got = {n: t.detach().clone() for n, t in got.items()}
    if not oracle:
        return got
    Pr = {n: t.clone().requires_grad_(True) for n, t in P.items()}
    Xr = [t.clone().requires_grad_(True) for t in Xs]
    Yr = [t.clone().requires_grad_(True) for t in Ys]
    Xpr = [t.clone().requires_grad_(True) for t in Xps]
    Ypr = [t.clone().requires_grad_(True) for t in Yps]
    oo, lo, ao, total, a0 = [], [], [], 0, 0
    for v in range(nv):
        o, lg, at = fo.x2y(Pr, "", Xr[v], Yr[v], Xpr[v], Ypr[v])
        n = lg.numel()
        total = (total + (o * gout[yl[v]:yl[v + 1]]).sum() + (lg.reshape(-1) * glog.reshape(-1)[a0:a0 + n]).sum() +
                 (at.reshape(-1) * gatt.reshape(-1)[a0:a0 + n]).sum())
        oo.append(o.detach())
        lo.append(lg.detach().reshape(-1))
        ao.append(at.detach().reshape(-1))
        a0 += n
    total.backward()
    ref = {"out": torch.cat(oo), "logit": torch.cat(lo), "attn": torch.cat(ao),
           "dX": torch.cat([t.grad for t in Xr]), "dY": torch.cat([t.grad for t in Yr]),
           "dXpos": torch.cat([t.grad for t in Xpr]), "dYpos": torch.cat([t.grad for t in Ypr])}
    ref.update({n: Pr[n].grad for n in P})
    for n, r in ref.items():
        tol = 1e-5 if n == "attn" else 2e-4 if n in P else 1e-4
        err = (got[n].double().cpu().reshape(r.shape) - r).abs().max().item()
        assert err <= tol * (1 + r.abs().max().item()), (n, err)
    return got


@pytest.mark.parametrize("direction,Ts", [("a2f", (700, 413)), ("f2a", (400, 330)), ("f2a", (4097, 330))])
def test_ragged_token_counts_in_one_call(direction, Ts):
    """Videos of 40 and 75 tokens in one call: the wide core, its LDS tile / slab rows sized by the widest
    video, the narrower video's blocks masked."""
    lib = nx.load()
    tk, fr = nx.int_array([0, 40, 115]), nx.int_array([0, Ts[0], Ts[0] + Ts[1]])
    xo, yo = (tk, fr) if direction == "a2f" else (fr, tk)
    want = 0 if sum(Ts) < 1024 else 1 if direction == "a2f" else 2    # (400 + 330 keys: segment level, grouped)
    assert lib.fx_x2y_core(base.H, 2, xo, yo, xo[2], yo[2]) == want
    _run_x2y(direction, (40, 75), Ts, oracle=True)
    fxf.check_device_status()


def _prof_count(lib, kind):
    ms, fl, by, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
    assert lib.fx_prof_collect(kind, ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by), ctypes.byref(n)) == 0
    return n.value


@pytest.mark.parametrize("direction,T,kinds", [("a2f", 4097, (3, 4)), ("f2a", 4097, (5,))])
def test_the_fused_core_ran(direction, T, kinds):
    """75 tokens: the fx_prof brackets of the fused cores count a call each -- the grouped GEMMs the call
    took before the wide variants open no bracket.  Frame level (>= 1024 rows): kinds 3 / 4 (a2f forward
    and backward) and 5 (f2a forward; its backward, kind 6, is counted in the child process of
    test_wide_f2a_fused_backward_vs_oracle, the wide f2a backward being opt-in).  Calls below 1024 rows
    (kinds 11 to 14) stay on the grouped GEMMs."""
    lib = nx.load()
    try:
        for k in kinds:
            assert lib.fx_prof_enable(k, 8) == 0
        _run_x2y(direction, (75,), (T,), oracle=False)
        counts = [_prof_count(lib, k) for k in kinds]
    finally:
        lib.fx_prof_disable()
    assert all(c >= 1 for c in counts), (kinds, counts)
    fxf.check_device_status()


@pytest.mark.parametrize("direction,nqs,Ts", [("a2f", (300, 97), (700, 413)), ("f2a", (300, 129), (4200, 413)),
                                              ("a2f", (40, 33), (700, 413)), ("f2a", (40, 33), (4200, 413))])
def test_wide_cores_are_deterministic(direction, nqs, Ts):
    """Two runs of one wide call (several row chunks of the a2f weight-side kernel; the f2a forward at 73
    chunks, its fused backward in the child process of test_wide_f2a_fused_backward_vs_oracle), and of the
    <= 64-row cores with ragged token counts (they share their phase bodies with the wide ones): every
    output and gradient bitwise equal."""
    a = _run_x2y(direction, nqs, Ts, oracle=False)
    b = _run_x2y(direction, nqs, Ts, oracle=False)
    for n in a:
        assert torch.equal(a[n], b[n]), n
    fxf.check_device_status()


if __name__ == "__main__":      # child of test_wide_f2a_fused_backward_vs_oracle: python tests/test_gpu_x2y_tokens.py f2a
    assert sys.argv[1] == "f2a"
    for nq, Ts in F2A_CASES:
        _checked("f2a", nq, Ts)
        print("ok f2a", nq, Ts, flush=True)
    _run_x2y("f2a", (40, 75), (400, 330), oracle=True)
    fxf.check_device_status()
    print("ok f2a ragged", flush=True)
    lib = nx.load()
    try:
        assert lib.fx_prof_enable(6, 8) == 0
        r1 = _run_x2y("f2a", (300, 129), (4200, 413), oracle=False)
        n6 = _prof_count(lib, 6)
    finally:
        lib.fx_prof_disable()
    assert n6 >= 1, n6
    r2 = _run_x2y("f2a", (300, 129), (4200, 413), oracle=False)
    for n in r1:
        assert torch.equal(r1[n], r2[n]), n
    fxf.check_device_status()
    print("ok f2a backward core ran, deterministic", flush=True)
