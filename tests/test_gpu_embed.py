"""The token embedding of a transcript input (csrc/embed.hip, fxf.token_embed) against float64 torch (GPU).

Forward: out[r] = W[ids[r]] + pe[pos[r]] is one fp32 add per element (error <= u |out|, u = 6e-8).
Backward: dW[c] sums at most 7 rows here in row order (error <= 7 u x the partial sums).  Both sit far
inside the bound of the issue, 1e-6 x (1 + max |ref|), which the tests assert.
"""
import numpy as np
import pytest
import torch

from factmx import functional as fxf
from factmx import native as nx

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _r(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def _close(got, ref, what):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs().max().item() if ref.numel() else 0.0
    assert err <= 1e-6 * (1.0 + ref.abs().max().item()), f"{what}: max error {err:.3e}"


# (ids, positions, C, A, with pe)
CASES = {
    "R=1": ([3], [0], 5, 32, True),
    "R=7 all ids equal": ([2] * 7, list(range(7)), 5, 32, True),
    "first and last class": ([0, 11, 0, 11, 5], list(range(5)), 12, 32, True),
    "A=33": ([2, 5, 9, 2, 5], list(range(5)), 12, 33, True),
    "A=256": ([2, 5, 9, 2, 5], list(range(5)), 12, 256, True),
    "two videos, positions restart": ([2, 5, 9, 2, 5, 1, 2, 1], [0, 1, 2, 3, 4, 0, 1, 2], 12, 32, True),
    "pe NULL": ([4, 1, 4, 0], None, 6, 40, False),
}


def _run(ids, pos, C, A, with_pe, leaf, seed=0, pre=None):
    """(out, dW, reference out, reference dW); ``leaf``: W is a leaf (the kernel accumulates into W.grad,
    which starts as ``pre`` if given), else a computed tensor (the kernel writes the whole gradient)."""
    R = len(ids)
    W64, pe64, g64 = _r(C, A, seed=seed), _r(16, 1, A, seed=seed + 1), _r(R, A, seed=seed + 2)
    W0 = W64.float().to(DEV).requires_grad_(True)
    if pre is not None:
        W0.grad = pre.float().to(DEV)
    W = W0 if leaf else W0 * 1.0
    pe = pe64.float().to(DEV) if with_pe else None
    out = fxf.token_embed(W, np.array(ids), pe, None if pos is None else np.array(pos))
    out.backward(g64.float().to(DEV))
    torch.cuda.synchronize()
    Wr = W64.float().double().requires_grad_(True)
    ref = Wr[torch.tensor(ids)]
    if with_pe:
        ref = ref + pe64.float().double()[torch.tensor(pos), 0]
    ref.backward(g64.float().double())
    return out, W0.grad, ref, Wr.grad


@pytest.mark.parametrize("leaf", [True, False], ids=["accumulate", "write"])
@pytest.mark.parametrize("name", list(CASES))
def test_forward_and_backward_match_float64(name, leaf):
    ids, pos, C, A, with_pe = CASES[name]
    out, dW, ref, dWr = _run(ids, pos, C, A, with_pe, leaf)
    _close(out, ref, name + " forward")
    _close(dW, dWr, name + " backward")
    absent = [c for c in range(C) if c not in ids]
    assert absent and (dW[absent] == 0).all(), "classes that do not occur must stay zero"


def test_accumulate_adds_to_an_existing_gradient():
    ids, pos, C, A, with_pe = CASES["two videos, positions restart"]
    pre = _r(C, A, seed=9)
    _, dW, _, dWr = _run(ids, pos, C, A, with_pe, leaf=True, pre=pre)
    _close(dW, dWr + pre.float().double(), "accumulated gradient")
    absent = [c for c in range(C) if c not in ids]
    assert torch.equal(dW[absent].cpu(), pre.float()[absent]), "rows of absent classes must be left alone"


def test_write_mode_overwrites_every_row():
    """accumulate = 0 on a buffer full of garbage: occurring classes get their sums, the others zeros."""
    lib = nx.load()
    ids = np.array([2, 5, 9, 2, 5], dtype=np.int32)
    C, A, R = 12, 33, 5
    coff, clist = fxf.token_csr(ids, C)
    tab = torch.from_numpy(np.concatenate([coff, clist])).to(DEV)
    dout = _r(R, A, seed=4).float().to(DEV)
    dW = torch.full((C, A), 7.5, device=DEV)
    p = tab.data_ptr()
    nx.check(lib.fx_token_embed_bwd(dout.data_ptr(), A, R, C, A, coff.ctypes.data, clist.ctypes.data, p,
                                    p + 4 * (C + 1), dW.data_ptr(), A, 0, nx.stream()), "fx_token_embed_bwd")
    ref = torch.zeros(C, A, dtype=torch.float64)
    ref.index_add_(0, torch.from_numpy(ids.astype(np.int64)), dout.double().cpu())
    _close(dW, ref, "write mode")
    assert (dW[[c for c in range(C) if c not in ids]] == 0).all()


def test_two_runs_are_bitwise_equal():
    ids, pos, C, A, with_pe = CASES["R=7 all ids equal"]
    a = _run(ids, pos, C, A, with_pe, leaf=True)
    b = _run(ids, pos, C, A, with_pe, leaf=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    ids, pos, C, A, with_pe = CASES["two videos, positions restart"]
    a = _run(ids, pos, C, A, with_pe, leaf=False)
    b = _run(ids, pos, C, A, with_pe, leaf=False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("bad", [-1, 12])
def test_an_out_of_range_id_is_refused_before_any_launch(bad):
    lib = nx.load()
    W = torch.zeros(12, 32, device=DEV, requires_grad=True)
    with pytest.raises((ValueError, nx.FactmxNativeError)):
        fxf.token_embed(W, np.array([2, bad, 5]))
    # the C entry itself: the host copy is checked first, nothing is enqueued (the device pointers are never read)
    ids = np.array([2, bad, 5], dtype=np.int32)
    out = torch.full((3, 32), 3.0, device=DEV)
    st = lib.fx_token_embed_fwd(W.data_ptr(), 32, 12, 32, ids.ctypes.data, None, out.data_ptr(), None, 3, None, 0, 0,
                                out.data_ptr(), 32, nx.stream())
    assert st != 0 and b"class id out of range" in lib.fx_last_error()
    torch.cuda.synchronize()
    assert (out == 3.0).all()
