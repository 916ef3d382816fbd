"""Fused clip_grad_norm_ + SGD on flat buffers (fx_sgd_step, factmx.optim.FusedSGD) against
torch.nn.utils.clip_grad_norm_ + torch.optim.SGD (scripts/train.py:219-221, :265-267) and against the float64
restatement sgd_cases._SgdRef, which test_optim_surface.py pins to torch in float64 (GPU).

Parameter bound: sgd_cases._SgdRef.tol, from the reference trajectory (two fp32 roundings per step in p, two in
buf accumulated geometrically, the clip coefficient's 2e-5).  Norm 1e-5 relative, clipped gradient rtol 1e-5
(atol 1e-7): test_gpu_optim.py's bounds.  Every case also asserts that the parameters moved by >= 100 x the
bound, so the bound never covers the whole update.
"""
import math

import pytest
import torch

from factmx import native as nx
from factmx.optim import FusedAdam, FusedSGD, build_optimizer
from sgd_cases import F32, _SgdRef

pytestmark = pytest.mark.gpu
DEV = "cuda"
LR = 1e-2


def _cat(ts):
    return torch.cat([t.detach().reshape(-1) for t in ts]).cpu()


def _check_step(step, opt, params, ref, norm, gc, clipped):
    """One step's comparisons; prints the figures before it asserts."""
    tol = ref.tol(F32(LR))
    err = (_cat(params).double() - ref.p).abs().max().item()
    print(f"step {step}: norm {opt.total_norm.item() if clipped else None} ref {norm}  param err {err:.3g} tol {tol:.3g}")
    if clipped:
        assert abs(opt.total_norm.item() - norm) <= 1e-5 * norm, (opt.total_norm.item(), norm)
    assert torch.allclose(_cat([p.grad for p in params]).double(), gc, rtol=1e-5, atol=1e-7), f"step {step}: clipped grad"
    assert err <= tol, f"step {step}: param err {err} > {tol}"
    if ref.momentum:
        berr = (opt.momentum_buffer.cpu().double() - ref.buf).abs().max().item()
        assert berr <= ref.buf_tol(), f"step {step}: momentum buffer err {berr} > {ref.buf_tol()}"
    else:
        assert opt.momentum_buffer is None, "momentum == 0 must not allocate a buffer"


def _check_moved(params, p0, ref):
    move = (_cat(params).double() - p0.double()).abs().max().item()
    print(f"moved {move:.3g} = {move / ref.tol(F32(LR)):.0f} x tol")
    assert move >= 100 * ref.tol(F32(LR)), (move, ref.tol(F32(LR)))


# ---------------------------------------------------------------------------------------------------------
# odd sizes exercise the scalar tail; (1,) a lone bias   (test_gpu_optim.py's list)
SHAPES = [(7, 5), (256, 256, 3), (1,), (513,), (33, 17)]


def _params(seed, shapes):
    # 0.1 x randn, the scale of initialised weights: with max_norm 0.5 over 197 718 elements a step moves an
    # element by ~lr x 3 x 4.6 x 3.7e-4 = 5e-5, and parameters of magnitude 4.6 (plain randn) would carry an
    # fp32 rounding bound of 2.2e-6 over 4 steps -- the update must be >= 100 x the bound
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter((0.1 * torch.randn(*s, generator=g)).to(DEV)) for s in shapes]


@pytest.mark.parametrize("max_norm,wd,momentum,gscale", [(10.0, 0.0, 0.9, 1.0), (10.0, 0.0, 0.9, 50.0),
                                                         (None, 0.01, 0.9, 1.0), (0.5, 0.0, 0.0, 3.0),
                                                         (None, 0.0, 0.0, 1.0), (0.5, 0.01, 0.009, 3.0)])
def test_fused_sgd_matches_torch(max_norm, wd, momentum, gscale):
    """fp32 torch.optim.SGD + clip_grad_norm_ on the same device, 4 steps; the bound comes from the float64
    trajectory of the same gradients."""
    ref, mine = _params(0, SHAPES), _params(0, SHAPES)
    p0 = _cat(mine)
    opt_ref = torch.optim.SGD(ref, lr=LR, momentum=momentum, weight_decay=wd)
    opt = FusedSGD(mine, lr=LR, momentum=momentum, weight_decay=wd, max_grad_norm=max_norm)
    traj = _SgdRef(p0, F32(LR), F32(momentum), F32(wd), F32(max_norm) if max_norm else None)
    g = torch.Generator().manual_seed(1)
    for step in range(4):
        grads = [torch.randn(*s, generator=g) * gscale for s in SHAPES]
        for p, gr in zip(ref, grads):
            p.grad = gr.to(DEV)
        for p, gr in zip(mine, grads):
            p.grad.copy_(gr)
        if max_norm:
            n_ref = torch.nn.utils.clip_grad_norm_(ref, max_norm)
        opt_ref.step()
        opt.step()
        torch.cuda.synchronize()
        traj.step(_cat(grads))
        tol = traj.tol()
        if max_norm:
            assert abs(opt.total_norm.item() - n_ref.item()) <= 1e-5 * n_ref.item()
        err = 0.0
        for a, b in zip(mine, ref):
            assert torch.allclose(a.grad, b.grad, rtol=1e-5, atol=1e-7), "clipped grad differs"
            err = max(err, (a.detach() - b.detach()).abs().max().item())
        print(f"step {step}: param err {err:.3g} tol {tol:.3g}")
        assert err <= tol, f"step {step}: param err {err} > {tol}"
        if momentum:
            bufs = torch.cat([opt_ref.state[p]["momentum_buffer"].reshape(-1) for p in ref])
            assert (opt.momentum_buffer - bufs).abs().max().item() <= traj.buf_tol()
    assert opt.step_count == 4 and (opt.momentum_buffer is None) == (momentum == 0)
    _check_moved(mine, p0, traj)


# ---------------------------------------------------------------------------------------------------------
# Launch-geometry edges on ONE flat buffer of n floats against _SgdRef, driven by the same fp32 gradients.
# (NPART = 1024 partial-sum blocks of ceil(n / NPART) elements each; sgd_kernel: n4 = n / 4 float4 groups over
# min(ceil(ceil(n / 4) / 256), 2048) blocks, then a scalar tail of n % 4 elements)
SGD_N = [
    1,          # n4 == 0: the scalar tail alone does the update; 1023 of the NPART partial-sum blocks are empty
    2,          # n4 == 0, two tail threads
    3,          # n4 == 0, the longest tail
    5,          # n4 == 1: one float4 group + a one-element tail; n < NPART
    1023,       # n < NPART: the last partial-sum block owns nothing; 255 groups + a tail of 3, one block
    1025,       # n > NPART: per = 2, blocks 513..1023 own nothing; 256 groups fill block 0, the second block idles
    2100003,    # ceil(n / 4) = 525 001 > 2048 blocks x 256 threads: the block cap holds and the grid-stride loop
                # takes a second pass (712 groups) + a tail of 3
]
GSCALE = 3.0


def _flat_case(n, steps, momentum=0.0, wd=0.0, max_norm=None, gscale=GSCALE, seed=0, schedule=None):
    """``schedule``: {step: fn(opt, ref)} run before that step (hyper-parameter changes through param_groups)."""
    g = torch.Generator().manual_seed(seed)
    p0 = torch.randn(n, generator=g)
    param = torch.nn.Parameter(p0.clone().to(DEV))
    opt = FusedSGD([param], lr=LR, momentum=momentum, weight_decay=wd, max_grad_norm=max_norm)
    assert (opt.momentum_buffer is None) == (momentum == 0)
    ref = _SgdRef(p0, F32(LR), F32(momentum), F32(wd), F32(max_norm) if max_norm else None)
    for step in range(steps):
        if schedule and step in schedule:
            schedule[step](opt, ref)
        grad = torch.randn(n, generator=g) * gscale
        param.grad.copy_(grad)
        opt.step()
        torch.cuda.synchronize()
        norm, gc = ref.step(grad)
        if not max_norm:
            assert torch.equal(param.grad.cpu(), grad), "no clipping: param.grad must be bitwise untouched"
        elif norm * (1 + 1e-5) + 1e-6 <= max_norm:   # (clear of the fp32 norm's own error)
            assert torch.equal(param.grad.cpu(), grad), "coef == 1: param.grad must be bitwise untouched"
        _check_step(step, opt, [param], ref, norm, gc, bool(max_norm))
    assert opt.step_count == steps
    _check_moved([param], p0, ref)
    return opt, ref


def _clip_level(n, gscale=GSCALE):
    """Half the expected gradient norm: the clip is active, and the per-element step keeps its size as n grows
    (a fixed max_norm = 1 at n = 2e6 would shrink it below the bound)."""
    return F32(0.5 * gscale * math.sqrt(n))


@pytest.mark.parametrize("momentum", [0.9, 0.0])
@pytest.mark.parametrize("n", SGD_N)
def test_fused_sgd_flat_sizes(n, momentum):
    """Every size with the clip active (for n = 1 on the steps where |g| > 1.5), 6 steps (3 at the largest size)."""
    _flat_case(n, 3 if n > 2000000 else 6, momentum=momentum, max_norm=_clip_level(n), seed=n)


@pytest.mark.parametrize("momentum", [0.9, 0.0])
@pytest.mark.parametrize("n", SGD_N)
def test_fused_sgd_flat_sizes_unclipped(n, momentum):
    """max_norm None: no partial-sum launch, a null workspace pointer in the kernel arguments, coef == 1."""
    _flat_case(n, 3 if n > 2000000 else 6, momentum=momentum, seed=n + 1)


@pytest.mark.parametrize("n", [1025, 2100003])
def test_fused_sgd_weight_decay_with_clipping(n):
    """The decay term is added to the CLIPPED gradient, before the momentum; param.grad holds the clipped gradient
    without it (_check_step compares .grad with the reference's clipped gradient)."""
    _flat_case(n, 3, momentum=0.009, wd=0.01, max_norm=_clip_level(n, 1.0), gscale=1.0, seed=5)


@pytest.mark.parametrize("momentum", [0.9, 0.0])
@pytest.mark.parametrize("n", [3, 1025])
def test_fused_sgd_norm_below_max_leaves_grad_bitwise(n, momentum):
    """||g|| < max_norm: coef == 1 and neither loop of sgd_kernel writes the gradient back."""
    opt, _ = _flat_case(n, 6, momentum=momentum, max_norm=1e4, gscale=1.0, seed=6)   # (_flat_case asserts it)
    assert opt.total_norm.item() < 1e4


def test_fused_sgd_momentum_raised_from_zero():
    """momentum 0 -> 0.9 through param_groups after two steps: the buffer appears at that step, zeroed, so the
    step's buf is d, as torch.optim.SGD creates its buffer at the first step that has momentum."""
    def raise_momentum(opt, ref):
        assert opt.momentum_buffer is None
        opt.param_groups[0]["momentum"] = 0.9
        ref.momentum, ref.buf = F32(0.9), torch.zeros_like(ref.p)
    opt, ref = _flat_case(1025, 5, max_norm=_clip_level(1025), seed=8, schedule={2: raise_momentum})
    assert opt.momentum == 0.9 and opt.momentum_buffer is not None


# ---------------------------------------------------------------------------------------------------------
# Learning-rate decay through param_groups (scripts/train.py:321-323)
def test_fused_sgd_lr_decay_through_param_groups():
    def decay(opt, ref):
        opt.param_groups[0]["lr"] *= 0.1
        ref.lr = F32(opt.lr)
    opt, ref = _flat_case(1025, 6, momentum=0.9, max_norm=_clip_level(1025), seed=9, schedule={3: decay})
    assert opt.lr == pytest.approx(LR * 0.1) and ref.lr == F32(LR * 0.1)


def test_fused_adam_lr_decay_through_param_groups():
    """The same schedule on FusedAdam against torch.optim.Adam, within test_gpu_optim.py's 2e-6 at lr 1e-3; the
    decayed steps move the parameters by ~1e-4 each, an undecayed step by ~1e-3."""
    shapes = [(33, 17), (513,), (1,)]
    gen = torch.Generator().manual_seed(0)
    init = [torch.randn(*s, generator=gen) for s in shapes]
    ref = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
    mine = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
    opt_ref = torch.optim.Adam(ref, lr=1e-3)
    opt = FusedAdam(mine, lr=1e-3, max_grad_norm=10.0)
    for step in range(6):
        if step == 3:
            for o in (opt_ref, opt):
                for group in o.param_groups:
                    group["lr"] = 1e-3 * 0.1
        before = _cat(mine)
        grads = [torch.randn(*s, generator=gen) for s in shapes]
        for p, gr in zip(ref, grads):
            p.grad = gr.to(DEV)
        for p, gr in zip(mine, grads):
            p.grad.copy_(gr)
        torch.nn.utils.clip_grad_norm_(ref, 10.0)
        opt_ref.step()
        opt.step()
        torch.cuda.synchronize()
        err = (_cat(mine) - _cat(ref)).abs().max().item()
        move = (_cat(mine) - before).abs().max().item()
        print(f"step {step}: err {err:.3g} move {move:.3g}")
        assert err <= 2e-6, f"step {step}: param err {err}"
        assert (move <= 2e-4) if step >= 3 else (move >= 5e-4), (step, move)
    assert opt.lr == 1e-3 * 0.1


# ---------------------------------------------------------------------------------------------------------
# The status guard, through the C ABI with a status word of the test's own (the library's word is not touched)
@pytest.mark.parametrize("momentum", [0.9, 0.0])
def test_sgd_step_status_guard(momentum):
    lib = nx.load()
    n = 1025
    gen = torch.Generator().manual_seed(12)
    p0, g0, b0 = (torch.randn(n, generator=gen) for _ in range(3))
    p, g = p0.to(DEV), (g0 * GSCALE).to(DEV)
    buf = b0.to(DEV) if momentum else None
    ws = torch.empty(lib.fx_grad_norm_workspace_floats(), device=DEV)
    norm = torch.zeros(1, device=DEV)
    max_norm = _clip_level(n)
    status = torch.ones(1, dtype=torch.int32, device=DEV)

    def call():
        nx.check(lib.fx_sgd_step(nx.ptr(p), nx.ptr(g), nx.ptr(buf), n, LR, momentum, 0.0, max_norm, nx.ptr(ws),
                                 nx.ptr(norm), nx.ptr(status), nx.stream()), "fx_sgd_step")
        torch.cuda.synchronize()
    call()                                          # status 1: every block returns before it touches anything
    assert torch.equal(p.cpu(), p0) and torch.equal(g.cpu(), g0 * GSCALE)
    assert buf is None or torch.equal(buf.cpu(), b0)
    status.zero_()
    call()                                          # status 0: the step is applied
    ref = _SgdRef(p0, F32(LR), F32(momentum), 0.0, max_norm)
    if momentum:
        ref.buf = b0.double()
    n_ref, gc = ref.step(g0 * GSCALE)
    ref.B = max(ref.B, b0.abs().max().item())
    assert n_ref > max_norm and abs(norm.item() - n_ref) <= 1e-5 * n_ref
    assert torch.allclose(g.cpu().double(), gc, rtol=1e-5, atol=1e-7)
    err = (p.cpu().double() - ref.p).abs().max().item()
    move = (p.cpu() - p0).abs().max().item()
    print(f"err {err:.3g} tol {ref.tol():.3g} move {move:.3g}")
    assert err <= ref.tol() and move >= 100 * ref.tol()
    assert status.item() == 0


# ---------------------------------------------------------------------------------------------------------
def test_fused_sgd_on_shared_grad_buffer():
    """FusedSGD over FlatGradReducer's gradient buffer: autograd accumulates into the views, the step reads them."""
    from factmx.dp import FlatGradReducer
    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Linear(13, 7), torch.nn.Tanh(), torch.nn.Linear(7, 3)).to(DEV)
    twin = torch.nn.Sequential(torch.nn.Linear(13, 7), torch.nn.Tanh(), torch.nn.Linear(7, 3)).to(DEV)
    twin.load_state_dict(net.state_dict())
    red = FlatGradReducer(net.parameters())
    opt = FusedSGD(net.parameters(), lr=LR, momentum=0.9, max_grad_norm=1.0, grad_flat=red.flat)
    assert opt.grad_flat is red.flat
    opt_ref = torch.optim.SGD(twin.parameters(), lr=LR, momentum=0.9)
    params = list(net.parameters())
    p0 = _cat(params)
    traj = _SgdRef(p0, F32(LR), F32(0.9), 0.0, 1.0)
    x, y = torch.randn(32, 13, device=DEV), torch.randn(32, 3, device=DEV) * 4
    for step in range(3):
        red.zero_grad()
        opt_ref.zero_grad()
        ((net(x) - y) ** 2).sum().backward()
        ((twin(x) - y) ** 2).sum().backward()
        grads = _cat([p.grad for p in params])
        n_ref = torch.nn.utils.clip_grad_norm_(twin.parameters(), 1.0)
        opt.step()
        opt_ref.step()
        torch.cuda.synchronize()
        traj.step(grads)
        assert n_ref.item() > 1.0 and abs(opt.total_norm.item() - n_ref.item()) <= 1e-5 * n_ref.item()
        err = (_cat(params) - _cat(twin.parameters())).abs().max().item()
        print(f"step {step}: err {err:.3g} tol {traj.tol():.3g}")
        assert err <= traj.tol(), f"step {step}: param err {err}"
    _check_moved(params, p0, traj)


def test_build_optimizer_sgd_trains_tiny_model():
    """cfg.optimizer = "SGD" end to end on the tiny FACT_CLIP fixture: two zero_grad -> forward -> backward ->
    step rounds through build_optimizer."""
    import paramgen as pg
    from helpers import load_fixture, tiny_meta, cfg_from_meta, tiny_inputs
    from factmx import functional as fxf
    from factmx.models.blocks import FACT_CLIP
    from factmx.models.loss import MatchCriterion
    meta = tiny_meta(load_fixture("tiny_clip"))
    cfg = cfg_from_meta(meta)
    cfg.optimizer = "SGD"
    feats, label, text = tiny_inputs(meta)
    net = FACT_CLIP(cfg, meta["D"], meta["C"], text_embeddings=torch.from_numpy(text).float())
    with torch.no_grad():
        for n, p in net.named_parameters():
            p.copy_(torch.from_numpy(pg.param_value(n, p.shape, meta["seed"])))
    net.mcriterion = MatchCriterion(cfg, meta["C"], [])
    net = net.to(DEV).train()
    opt = build_optimizer(cfg, net.parameters())
    assert type(opt) is FusedSGD and (opt.lr, opt.momentum, opt.max_grad_norm) == (cfg.lr, cfg.momentum, 10.0)
    seqs, labs = [torch.from_numpy(feats).float().to(DEV)], [torch.from_numpy(label).to(DEV)]
    for _ in range(2):
        w0 = opt.flat.clone()
        opt.zero_grad()
        loss, _ = net(seqs, labs, compute_loss=True)
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        assert torch.isfinite(loss).item() and torch.isfinite(opt.flat).all().item()
        assert not torch.equal(opt.flat, w0), "the step changed no parameter"
        assert math.isfinite(opt.total_norm.item()) and opt.total_norm.item() > 0
    fxf.check_device_status()                       # raises if a kernel of either step set the status word
    assert opt.step_count == 2
