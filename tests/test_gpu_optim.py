"""Fused clip_grad_norm_ + Adam on flat buffers (fx_adam_step) vs torch.nn.utils.clip_grad_norm_ +
torch.optim.Adam (scripts/train.py:265-267) on the same parameters and gradients (GPU)."""
import pytest
import torch

from factmx.optim import FusedAdam, clip_grad_norm_flat_

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _params(seed, shapes):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(*s, generator=g).to(DEV)) for s in shapes]


# odd sizes exercise the scalar tail; (1,) a lone bias
SHAPES = [(7, 5), (256, 256, 3), (1,), (513,), (33, 17)]


@pytest.mark.parametrize("max_norm,wd,gscale", [(10.0, 0.0, 1.0), (10.0, 0.0, 50.0), (None, 0.01, 1.0),
                                                (0.5, 0.0, 3.0)])
def test_fused_adam_matches_torch(max_norm, wd, gscale):
    ref = _params(0, SHAPES)
    mine = _params(0, SHAPES)
    opt_ref = torch.optim.Adam(ref, lr=1e-3, weight_decay=wd)
    opt = FusedAdam(mine, lr=1e-3, weight_decay=wd, max_grad_norm=max_norm)
    g = torch.Generator().manual_seed(1)
    for step in range(4):
        grads = [torch.randn(*s, generator=g).to(DEV) * gscale for s in SHAPES]
        for p, gr in zip(ref, grads):
            p.grad = gr.clone()
        for p, gr in zip(mine, grads):
            p.grad.copy_(gr)
        if max_norm:
            n_ref = torch.nn.utils.clip_grad_norm_(ref, max_norm)
        opt_ref.step()
        opt.step()
        torch.cuda.synchronize()
        if max_norm:
            assert abs(opt.total_norm.item() - n_ref.item()) <= 1e-5 * n_ref.item()
        for a, b in zip(mine, ref):
            assert torch.allclose(a.grad, b.grad, rtol=1e-5, atol=1e-7), "clipped grad differs"
            err = (a.detach() - b.detach()).abs().max().item()
            assert err <= 2e-6, f"step {step}: param err {err}"


def test_clip_grad_norm_flat():
    g = torch.Generator().manual_seed(3)
    flat = (torch.randn(100003, generator=g) * 0.1).to(DEV)
    ref = flat.clone()
    n_ref = torch.linalg.vector_norm(ref)
    ref.mul_(torch.clamp(1.0 / (n_ref + 1e-6), max=1.0))
    n = clip_grad_norm_flat_(flat, 1.0)
    torch.cuda.synchronize()
    assert abs(n.item() - n_ref.item()) <= 1e-5 * n_ref.item()
    assert torch.allclose(flat, ref, rtol=1e-5, atol=1e-8)


# ---------------------------------------------------------------------------------------------------------
# Launch-geometry edges of csrc/optim.hip on ONE flat buffer of n floats, against a float64 restatement of the
# update on the CPU driven by the same fp32 gradients.  Bounds are this file's own: parameters 2e-6 absolute at
# lr 1e-3, norm 1e-5 relative, clipped gradient rtol 1e-5 (atol 1e-7).
#
# n: what it reaches (NPART = 1024 partial-sum blocks of ceil(n / NPART) elements each; adam_kernel: n4 = n / 4
# float4 groups over min(ceil(ceil(n / 4) / 256), 2048) blocks, then a scalar tail of n % 4 elements)
ADAM_N = [
    1,          # n4 == 0: the scalar tail alone does the update; 1023 of the NPART partial-sum blocks are empty
    2,          # n4 == 0, two tail threads
    3,          # n4 == 0, the longest tail
    5,          # n4 == 1: one float4 group + a one-element tail; n < NPART (per = 1, blocks 5..1023 own nothing)
    1023,       # n < NPART: per = 1, the last block owns nothing; n4 = 255 groups + a tail of 3, one block
    1025,       # n > NPART: per = 2, blocks 513..1023 own nothing; n4 = 256 fills block 0, whose thread 0 also
                # takes the one-element tail; the launch's second block (ceil(n / 4) = 257 groups) finds no work
    2100003,    # ceil(n / 4) = 525 001 > 2048 blocks x 256 threads = 524 288: the 2048-block cap of
                # fx_adam_step_checked holds and the grid-stride loop takes a second pass (712 groups) + a tail of 3
]


def F32(v):
    """The value a float argument of the C ABI holds."""
    return float(torch.tensor(v, dtype=torch.float32).item())


LR, B1, B2, EPS = F32(1e-3), F32(0.9), F32(0.999), F32(1e-8)


class _AdamRef:
    """The header comment of optim.hip in float64: clip by min(max_norm / (norm + 1e-6), 1), L2 weight decay
    g += wd p, m = m + (1 - b1)(g - m), v = b2 v + (1 - b2) g g, p -= lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps),
    bias corrections 1 - beta^step in double on the host."""

    def __init__(self, p, m=None, v=None, step=0, wd=0.0, max_norm=None):
        self.p = p.double().clone()
        self.m = torch.zeros_like(self.p) if m is None else m.double().clone()
        self.v = torch.zeros_like(self.p) if v is None else v.double().clone()
        self.t, self.wd, self.max_norm = step, F32(wd), (F32(max_norm) if max_norm else None)

    def step(self, g):
        """g: the fp32 gradient.  Returns (norm, the clipped gradient) as clip_grad_norm_ leaves them."""
        g = g.double()
        norm = g.norm().item()
        if self.max_norm:
            g = g * min(self.max_norm / (norm + 1e-6), 1.0)
        ge = g + self.wd * self.p if self.wd else g
        self.t += 1
        self.m = self.m + (1.0 - B1) * (ge - self.m)
        self.v = B2 * self.v + (1.0 - B2) * ge * ge
        bc1, bc2 = 1.0 - B1 ** self.t, 1.0 - B2 ** self.t
        self.p = self.p - (LR / bc1) * (self.m / (self.v.sqrt() / bc2 ** 0.5 + EPS))
        return norm, g


def _flat_case(n, steps, wd=0.0, max_norm=None, gscale=1.0, step0=0, seed=0):
    g = torch.Generator().manual_seed(seed)
    p0 = torch.randn(n, generator=g)
    param = torch.nn.Parameter(p0.clone().to(DEV))
    opt = FusedAdam([param], lr=1e-3, weight_decay=wd, max_grad_norm=max_norm)
    m0 = v0 = None
    if step0:   # a state as after step0 steps, set directly: the next step's bias corrections are step0 + 1's
        m0, v0 = torch.randn(n, generator=g) * 0.1, torch.rand(n, generator=g) * 0.01 + 1e-4
        opt.step_count = step0
        opt.exp_avg.copy_(m0)
        opt.exp_avg_sq.copy_(v0)
    ref = _AdamRef(p0, m0, v0, step0, wd, max_norm)
    for step in range(steps):
        grad = torch.randn(n, generator=g) * gscale
        param.grad.copy_(grad)
        opt.step()
        torch.cuda.synchronize()
        norm, gc = ref.step(grad)
        if max_norm:
            assert abs(opt.total_norm.item() - norm) <= 1e-5 * norm, (opt.total_norm.item(), norm)
            if norm * (1 + 1e-5) + 1e-6 <= max_norm:   # (clear of the fp32 norm's own error)
                assert torch.equal(param.grad.cpu(), grad), "coef == 1: param.grad must be bitwise untouched"
        else:
            assert torch.equal(param.grad.cpu(), grad), "no clipping: param.grad must be bitwise untouched"
        assert torch.allclose(param.grad.cpu().double(), gc, rtol=1e-5, atol=1e-7), f"step {step}: clipped grad"
        err = (param.detach().cpu().double() - ref.p).abs().max().item()
        assert err <= 2e-6, f"step {step}: param err {err}"
    assert opt.step_count == step0 + steps
    return opt, ref


@pytest.mark.parametrize("n", ADAM_N)
def test_fused_adam_flat_sizes(n):
    """Every size with the clip active (randn x 3 gradients against max_norm 1: coef < 1 for n >= 2 in practice, for
    n = 1 on the steps where |g| > 1), 6 steps (3 at the largest size)."""
    _flat_case(n, 3 if n > 2000000 else 6, max_norm=1.0, gscale=3.0, seed=n)


@pytest.mark.parametrize("n", ADAM_N)
def test_fused_adam_flat_sizes_unclipped(n):
    """max_norm None: no partial-sum launch, a null workspace pointer in the kernel arguments, coef == 1."""
    _flat_case(n, 3 if n > 2000000 else 6, seed=n + 1)


# 1025: two blocks, the tail in the second; 2100003: the second grid-stride pass
@pytest.mark.parametrize("n", [1025, 2100003])
def test_fused_adam_weight_decay_with_clipping(n):
    """Weight decay and clipping together: the decay term is added to the CLIPPED gradient, and param.grad holds
    the clipped gradient without the decay term."""
    _flat_case(n, 3, wd=0.01, max_norm=0.5, gscale=1.0, seed=5)


@pytest.mark.parametrize("n", [3, 1025])
def test_fused_adam_norm_below_max_leaves_grad_bitwise(n):
    """||g|| < max_norm: coef == 1 and neither loop of adam_kernel writes the gradient back."""
    opt, _ = _flat_case(n, 6, max_norm=1e4, gscale=1.0, seed=6)   # (_flat_case asserts the bitwise equality)
    assert opt.total_norm.item() < 1e4


@pytest.mark.parametrize("wd,max_norm", [(0.0, None), (0.01, 0.5)])
def test_fused_adam_step_1000_bias_corrections(wd, max_norm):
    """The 1000th step from a state set directly (step counter 999, non-zero moments): bc1 = 1 - 0.9^1000 = 1 to
    fp32, bc2 = 1 - 0.999^1000 = 0.632 -- a wrong exponent or a float pow would show in the parameter."""
    opt, _ = _flat_case(1025, 1, wd=wd, max_norm=max_norm, step0=999, seed=7)
    assert opt.step_count == 1000


@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("n", ADAM_N)
def test_grad_norm_and_clip_scale_flat_sizes(n, clip):
    """fx_grad_norm + fx_clip_grad_scale against the float64 norm: clipped to half the norm, or (max_norm above
    the norm) bitwise untouched."""
    g = torch.Generator().manual_seed(100 + n)
    g0 = torch.randn(n, generator=g) * 0.5
    n_ref = g0.double().norm().item()
    max_norm = F32(0.5 * n_ref if clip else 2.0 * n_ref + 1.0)
    flat = g0.clone().to(DEV)
    norm = clip_grad_norm_flat_(flat, max_norm)
    torch.cuda.synchronize()
    assert abs(norm.item() - n_ref) <= 1e-5 * n_ref
    if clip:
        ref = g0.double() * min(max_norm / (n_ref + 1e-6), 1.0)
        assert torch.allclose(flat.cpu().double(), ref, rtol=1e-5, atol=1e-8)
    else:
        assert torch.equal(flat.cpu(), g0)
