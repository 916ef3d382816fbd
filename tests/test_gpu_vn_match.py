"""fx_vn_match_cost (csrc/vnloss.hip): the matching cost of a verb/noun video from the token heads and
the segment-level attention (GPU).

Reference: the float64 restatement of loss.py:108-153 / 91-106 on the materialised tensors, the
frames x tokens x segments cube included (tests/vn_cases.py; computed on the device in float64).
Bound: every cost entry within 2e-5 x (1 + max|ref|), DESIGN.md section 7m's bound; the same restatement
in float32 on the CPU sits at most 1/3 of it from float64 over these cases (section 7n).
"""
import numpy as np
import pytest
import torch

from factmx import functional as fxf
import vn_cases as vc

pytestmark = pytest.mark.gpu
DEV = "cuda"

HEADS = [(5, 7, 12), (98, 301, 4000)]
SHAPES = [(T, Q, G) for T in (67, 700) for Q in (1, 5, 300) for G in (1, 7, 300) if G <= T]


def kernel_cost(case, attn, pc, a2fc, st=None, en=None):
    m = fxf.VerbNounMap(case["vids"], case["nids"])
    i32 = lambda a: None if a is None else torch.from_numpy(np.asarray(a, dtype=np.int32)).to(DEV)   # noqa: E731
    return fxf.vn_match_cost(case["acl"].to(DEV), attn.to(DEV), m, i32(case["gs"]), i32(case["ge"]), i32(case["gl"]),
                             case["T"], pc, a2fc, seg_start=i32(st), seg_end=i32(en))


def check(got, ref, what):
    assert got.shape == ref.shape and got.dtype == torch.float32, what
    assert bool(torch.isfinite(got).all()), what
    err = float((got.double() - ref).abs().max())
    lim = vc.BOUND * (1.0 + float(ref.abs().max()))
    print(f"{what}: max err {err:.3e} (bound {lim:.3e})")
    assert err <= lim, what


@pytest.mark.parametrize("V,N,A", HEADS)
@pytest.mark.parametrize("T,Q,G", SHAPES)
def test_cost_against_float64_cube(T, Q, G, V, N, A):
    pc, a2fc = 0.2, 1.0
    case = vc.match_case(T, Q, G, V, N, A, seed=T + 3 * Q + 7 * G)
    rng = np.random.default_rng(T + Q + G)
    zero = Q // 2 if Q >= 5 else None
    for kind in ("one", "frames", "rand"):
        st, en = vc.tdu_segments(T, case["gs"], case["ge"], kind, rng)
        if kind == "rand" and G >= 7:
            meet = [int(((case["gs"] <= b) & (case["ge"] >= a)).sum()) for a, b in zip(st, en)]
            inside = [bool(((st <= a) & (en >= b)).any()) for a, b in zip(case["gs"], case["ge"])]
            assert max(meet) >= 3 and any(inside), "TDU segments over several ground-truth segments and around one"
        seg, frame = vc.seg_attention(case, st, en, zero_token=zero)
        ref = vc.ref_cost(case, frame, pc, a2fc, device=DEV)
        check(kernel_cost(case, seg, pc, a2fc, st, en), ref, f"segment-level S={len(st)}")
        if kind != "one":
            check(kernel_cost(case, frame, pc, a2fc), ref, f"frame-level S={len(st)}")
        if zero is not None and a2fc:      # the silent token: IoU 0 (its cost is the probability term alone)
            only_p = vc.ref_cost(case, frame, pc, 0.0, device=DEV)
            assert float((ref[zero] - only_p[zero]).abs().max()) == 0.0


def test_single_token_without_attention():
    """Q = 1 and attention zero on every frame: union = len_s, IoU 0, no NaN."""
    case = vc.match_case(67, 1, 7, 5, 7, 12, seed=4)
    st, en = vc.tdu_segments(67, case["gs"], case["ge"], "rand", np.random.default_rng(0))
    seg, frame = vc.seg_attention(case, st, en, zero_token=0)
    ref = vc.ref_cost(case, frame, 0.2, 1.0, device=DEV)
    check(kernel_cost(case, seg, 0.2, 1.0, st, en), ref, "segment-level")
    check(kernel_cost(case, frame, 0.2, 1.0), ref, "frame-level")


@pytest.mark.parametrize("pc,a2fc", [(0.0, 1.0), (0.2, 0.0)])
def test_one_coefficient_zero(pc, a2fc):
    case = vc.match_case(700, 5, 7, 98, 301, 4000, seed=9)
    st, en = vc.tdu_segments(700, case["gs"], case["ge"], "rand", np.random.default_rng(1))
    seg, frame = vc.seg_attention(case, st, en)
    ref = vc.ref_cost(case, frame, pc, a2fc, device=DEV)
    check(kernel_cost(case, seg, pc, a2fc, st, en), ref, f"pc={pc} a2fc={a2fc}")
    check(kernel_cost(case, frame, pc, a2fc), ref, f"frame-level pc={pc} a2fc={a2fc}")


def test_two_runs_are_bitwise_equal_and_no_rows():
    case = vc.match_case(700, 300, 300, 98, 301, 4000, seed=2)
    st, en = vc.tdu_segments(700, case["gs"], case["ge"], "rand", np.random.default_rng(2))
    seg, frame = vc.seg_attention(case, st, en)
    a, b = kernel_cost(case, seg, 0.2, 1.0, st, en), kernel_cost(case, seg, 0.2, 1.0, st, en)
    assert torch.equal(a, b)
    a, b = kernel_cost(case, frame, 0.2, 1.0), kernel_cost(case, frame, 0.2, 1.0)
    assert torch.equal(a, b)
    with pytest.raises(ValueError):         # attention for another token count is refused before any launch
        fxf.vn_match_cost(case["acl"].to(DEV)[:5], seg.to(DEV), fxf.VerbNounMap(case["vids"], case["nids"]),
                          torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32),
                          torch.zeros(1, dtype=torch.int32), 700, 0.2, 1.0)


@pytest.mark.parametrize("T,Q,G,V,N,A", [(67, 5, 7, 5, 7, 12), (700, 300, 7, 5, 7, 12), (700, 300, 300, 98, 301, 4000),
                                         (700, 16, 300, 5, 7, 12)])
def test_match_equals_the_float64_match(T, Q, G, V, N, A):
    """The inputs leave no near-tie (the float64 match survives moving every entry by +- the bound, two
    seeded sign patterns); the kernel's cost then gives the same o2o and o2m pairs."""
    case = vc.match_case(T, Q, G, V, N, A, seed=5, structured=True)
    st, en = vc.tdu_segments(T, case["gs"], case["ge"], "rand", np.random.default_rng(3))
    seg, frame = vc.seg_attention(case, st, en)
    ref = vc.ref_cost(case, frame, 0.2, 1.0, device=DEV)
    lim = vc.BOUND * (1.0 + float(ref.abs().max()))
    assert vc.match_is_stable(ref, case["gl"], lim), "the test's inputs hold a near-tie"
    want = vc.matches(ref.cpu().numpy(), case["gl"])
    for got in (kernel_cost(case, seg, 0.2, 1.0, st, en), kernel_cost(case, frame, 0.2, 1.0)):
        assert vc.matches(got.double().cpu().numpy(), case["gl"]) == want


def test_no_cube_sized_allocation():
    T, Q, G = 2048, 300, 130
    cube = T * Q * G * 4
    case = vc.match_case(T, Q, G, 98, 301, 4000, seed=6)
    st, en = vc.tdu_segments(T, case["gs"], case["ge"], "rand", np.random.default_rng(4))
    seg, _ = vc.seg_attention(case, st, en)
    m = fxf.VerbNounMap(case["vids"], case["nids"])
    m.tables(torch.device(DEV, torch.cuda.current_device()))
    args = [torch.from_numpy(np.asarray(case[k], dtype=np.int32)).to(DEV) for k in ("gs", "ge", "gl")]
    sti, eni = (torch.from_numpy(x).to(DEV) for x in (st, en))
    acl, seg = case["acl"].to(DEV), seg.to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    cost = fxf.vn_match_cost(acl, seg, m, *args, T, 0.2, 1.0, seg_start=sti, seg_end=eni)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"vn_match_cost at T={T} Q={Q} G={G}: peak rise {rise / 1e3:.1f} KB (one cube {cube / 1e6:.0f} MB)")
    assert tuple(cost.shape) == (Q, G) and rise < cube / 10
