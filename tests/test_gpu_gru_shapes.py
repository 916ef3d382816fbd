"""Launch-geometry edges of the BiGRU recurrence kernels (csrc/gru.hip) against the float64 oracle (GPU).

Each direction of a sequence runs on NW = 16 workgroups of U = ceil(Hh / NW) <= MAXU hidden units each; in the
forward, wave wv of a workgroup owns the KCH = 64 wide chunk wv of the state.  tests/test_gpu_kernels.py's
test_gru_bidirectional has Hh in {256, 32, 24}: workgroups that are full or empty, chunks that are full or
empty, one sequence.  Here: partly filled workgroups (Hh % U != 0), partial chunks (Hh % 64 != 0), Hh = 1 and odd
Hh (the gi + 3 Hh and per-direction `saved` slices handed to the GEMMs are then not 16-byte aligned), one-row
sequences inside a ragged batch, and more than MAXSEQ = 32 sequences (the launcher chunks and offsets the granule
area per chunk).  Driven through fxf.gru on an nn.GRU(In, Hh, 1, bidirectional=True); the reference is fo.gru per
sequence, concatenated, on the exact fp32 parameter and input values.  Tolerances are test_gru_bidirectional's:
y at 2e-5 + 2e-5 max|ref|, gradients at 1e-4 + 1e-4 max|ref|."""
import pytest
import torch

from factmx import functional as fxf
from oracle import fact_oracle as fo

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _r(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64).float().double()


def _close(a, b, rtol=2e-5, atol=2e-5, what=""):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert torch.isfinite(a).all(), f"{what}: non-finite values"
    err = (a - b).abs().max().item()
    ref = b.abs().max().item()
    assert err <= atol + rtol * ref, f"{what}: max err {err:.3e} (ref max {ref:.3e})"


def _offsets(lens):
    off = [0]
    for n in lens:
        off.append(off[-1] + n)
    return off


def _module(In, Hh, seed=0):
    torch.manual_seed(seed)
    ref = torch.nn.GRU(In, Hh, 1, bidirectional=True)
    mod = torch.nn.GRU(In, Hh, 1, bidirectional=True).to(DEV)
    mod.load_state_dict(ref.state_dict())
    return mod, {n: p.detach().double().requires_grad_(True) for n, p in ref.named_parameters()}


def _gpu(mod, x, g, lens, relu):
    for p in mod.parameters():
        p.grad = None
    xd = x.float().to(DEV).requires_grad_(True)
    y = fxf.gru(mod, xd, seq_off=None if lens is None else _offsets(lens), relu=relu)
    (y * g.float().to(DEV)).sum().backward()
    torch.cuda.synchronize()
    fxf.check_device_status()       # no workgroup gave up waiting for a peer, forward or backward
    out = {"y": y.detach().cpu(), "dx": xd.grad.detach().cpu()}
    for n, p in mod.named_parameters():
        out[n] = p.grad.detach().cpu().clone()
    return out


def _case(In, Hh, lens, relu=False, S=None, seed=0):
    """lens None: one sequence of S rows through the seq_off = None entry; else a ragged batch."""
    rows = S if lens is None else sum(lens)
    mod, P = _module(In, Hh, seed)
    x, g = _r(rows, In, seed=seed + 28), _r(rows, 2 * Hh, seed=seed + 29)
    out = _gpu(mod, x, g, lens, relu)
    xr = x.clone().requires_grad_(True)
    off = _offsets([rows] if lens is None else lens)
    yr = torch.cat([fo.gru(P, "", xr[a:b], 1) for a, b in zip(off[:-1], off[1:])], 0)
    if relu:
        # the reference gates with the GPU's own y > 0: an output within fp32 noise of 0 may land on either side,
        # and that one element's gradient is then dout vs 0 all the way back through the recurrence
        gate = out["y"] > 0
        assert gate.any() and (~gate).any(), "relu case needs both signs"
        yr = yr * gate.double()
    (yr * g).sum().backward()
    _close(out["y"], yr, what="gru y")
    _close(out["dx"], xr.grad, rtol=1e-4, atol=1e-4, what="gru dx")
    for n in P:
        _close(out[n], P[n].grad, rtol=1e-4, atol=1e-4, what=f"gru d{n}")
    return mod, x, g, out


# One sequence, (S, In, Hh).  U = ceil(Hh / NW); workgroup j owns units [j U, j U + U) below Hh.
SINGLE = [
    (2, 8, 1),       # Hh = 1: U = 1, workgroup 0 holds the only unit, 15 are empty; wave 0's chunk is 1 of KCH
    (3, 20, 17),     # U = 2: workgroup 8 is half filled (unit 16), 9..15 empty; odd Hh: unaligned GEMM slices
    (9, 64, 100),    # U = 7: workgroup 14 holds 2 units (98, 99), 15 none; wave 1's chunk is 36 of KCH, waves 2, 3 none
    (9, 64, 200),    # U = 13: the last workgroup holds 5 units (195..199); wave 3's chunk is 8 of KCH
    (5, 32, 255),    # U = MAXU = 16: every workgroup full but the last, one unit short; wave 3's chunk is 63; odd Hh
]


@pytest.mark.parametrize("S,In,Hh", SINGLE)
def test_gru_single_sequence_shapes(S, In, Hh):
    _case(In, Hh, None, S=S, seed=Hh)


# Ragged batches: one launch of 2 NW workgroups per sequence, at most MAXSEQ = 32 sequences per launch.
RAGGED = {
    "4seq": (1, 6, 2, 1),              # one-row sequences first and last (no exchange at all: S = 1 skips it)
    "33seq": (1, 2, 3, 4) * 8 + (1,),  # MAXSEQ + 1: a second launch of ONE sequence at granule offset 32
    "40seq": (3, 1) * 20,              # two launches of 32 and 8 sequences
}


# Hh = 100: partly filled workgroups and chunks in every sequence; Hh = 256: NW x MAXU, the largest granule area;
# Hh = 17: odd, so the backward's tables ahead of its sync area hold an odd number of floats -- the 8-byte granules
# sat on a 4-byte boundary there and several sequences polling at once read torn epoch / value pairs
# (test_gru_ragged_relu[17] first showed it: dx off by 3e-2); the launchers now refuse an unaligned sync area
@pytest.mark.parametrize("Hh", [100, 256, 17])
@pytest.mark.parametrize("name", list(RAGGED))
def test_gru_ragged_batches(name, Hh):
    lens = RAGGED[name]
    mod, x, g, out = _case(64, Hh, lens, seed=len(lens))
    if name == "33seq":
        # the sync area is zeroed per call and the epochs restart: a second call gives the same bits
        again = _gpu(mod, x, g, lens, False)
        for k in out:
            assert torch.equal(out[k], again[k]), (k, (out[k] - again[k]).abs().max().item())


@pytest.mark.parametrize("Hh", [100, 17])
def test_gru_ragged_relu(Hh):
    """relu(GRU(x)) folded into the recurrence kernels, on a ragged batch with one-row sequences."""
    _case(64, Hh, (1, 6, 2, 1, 5), relu=True, seed=3)
