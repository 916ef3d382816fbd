"""The optimizer surface without a GPU: the float64 SGD restatement the GPU tests compare with against
torch.optim.SGD + clip_grad_norm_, build_optimizer(cfg), param_groups on FusedSGD / FusedAdam, and
fx_sgd_step's host-side argument checks (which run before any HIP call)."""
import ctypes
import itertools
import os
import re
import subprocess

import pytest
import torch

from factmx import native as nx
from factmx.configs import get_cfg_defaults
from factmx.optim import FusedAdam, FusedSGD, build_optimizer
from sgd_cases import _SgdRef

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "factmx.h")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(nx.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "fact-clip_amd", "csrc"), "-j8"], check=True,
                       stdout=subprocess.DEVNULL)
    return nx.load()


# ---------------------------------------------------------------------------------------------------------
# _SgdRef == torch.optim.SGD + clip_grad_norm_ in float64 (first-step buf = d, decay added after the clip and
# before momentum, clipped gradient left in .grad, pre-clip norm returned)
SHAPES = [(7, 5), (3,), (1,), (4, 3, 2)]


@pytest.mark.parametrize("momentum,wd,clipped", list(itertools.product([0.0, 0.009, 0.9], [0.0, 0.01], [True, False])))
def test_sgd_ref_matches_torch_float64(momentum, wd, clipped):
    gen = torch.Generator().manual_seed(11)
    params = [torch.nn.Parameter(torch.randn(*s, generator=gen, dtype=torch.float64)) for s in SHAPES]
    lr, max_norm = 0.1, (2.0 if clipped else None)     # ||g|| ~ sqrt(63) x 1.5: the clip is active every step
    opt = torch.optim.SGD(params, lr=lr, momentum=momentum, weight_decay=wd)
    ref = _SgdRef(torch.cat([p.detach().reshape(-1) for p in params]), lr, momentum, wd, max_norm)

    def close(a, b, what):
        assert (a - b).abs().max().item() <= 1e-12 * b.abs().max().item(), what

    for step in range(5):
        grads = [torch.randn(*s, generator=gen, dtype=torch.float64) * 1.5 for s in SHAPES]
        for p, g in zip(params, grads):
            p.grad = g.clone()
        if clipped:
            n_t = torch.nn.utils.clip_grad_norm_(params, max_norm).item()
        opt.step()
        norm, gc = ref.step(torch.cat([g.reshape(-1) for g in grads]))
        if clipped:
            assert norm > max_norm and abs(norm - n_t) <= 1e-12 * n_t
        close(gc, torch.cat([p.grad.reshape(-1) for p in params]), f"step {step}: gradient left in .grad")
        close(ref.p, torch.cat([p.detach().reshape(-1) for p in params]), f"step {step}: parameters")
        if momentum:
            close(ref.buf, torch.cat([opt.state[p]["momentum_buffer"].reshape(-1) for p in params]),
                  f"step {step}: momentum buffer")
        else:
            assert ref.buf is None and "momentum_buffer" not in opt.state[params[0]]


# ---------------------------------------------------------------------------------------------------------
# build_optimizer (scripts/train.py:219-224 + :266) on CPU parameters: the constructors only load the library
# and size buffers
def _cpu_params():
    gen = torch.Generator().manual_seed(0)
    return [torch.nn.Parameter(torch.randn(*s, generator=gen)) for s in [(5, 3), (4,)]]


def test_build_optimizer_default_config_is_sgd(lib):
    opt = build_optimizer(get_cfg_defaults(), _cpu_params())
    assert type(opt) is FusedSGD
    assert (opt.lr, opt.momentum, opt.weight_decay, opt.max_grad_norm) == (0.1, 0.009, 0.0, 10.0)
    assert opt.momentum_buffer is not None and opt.momentum_buffer.shape == opt.flat.shape
    assert not opt.momentum_buffer.any() and opt.step_count == 0


def test_build_optimizer_adam(lib):
    cfg = get_cfg_defaults()
    cfg.optimizer = "Adam"
    cfg.weight_decay = 0.01
    opt = build_optimizer(cfg, _cpu_params())
    assert type(opt) is FusedAdam
    assert (opt.lr, opt.weight_decay, opt.max_grad_norm) == (0.1, 0.01, 10.0)
    assert (opt.betas, opt.eps) == ((0.9, 0.999), 1e-8)          # torch.optim.Adam's defaults


@pytest.mark.parametrize("name", ["SGD", "Adam"])
def test_build_optimizer_no_clipping(lib, name):
    cfg = get_cfg_defaults()
    cfg.optimizer = name
    cfg.clip_grad_norm = 0
    assert build_optimizer(cfg, _cpu_params()).max_grad_norm is None


def test_build_optimizer_unknown_name(lib):
    cfg = get_cfg_defaults()
    cfg.optimizer = "RMSprop"
    with pytest.raises(ValueError, match="RMSprop"):
        build_optimizer(cfg, _cpu_params())


def test_build_optimizer_shares_grad_flat(lib):
    params = _cpu_params()
    flat = torch.zeros(sum(p.numel() for p in params))
    off = 0
    for p in params:
        p.grad = flat[off:off + p.numel()].view_as(p)
        off += p.numel()
    opt = build_optimizer(get_cfg_defaults(), params, grad_flat=flat)
    assert opt.grad_flat is flat
    params[0].grad = torch.zeros_like(params[0])               # no longer a view into the flat buffer
    with pytest.raises(ValueError, match="FusedSGD: parameter .grad must be views into grad_flat"):
        FusedSGD(params, lr=0.1, grad_flat=flat)


def test_sgd_without_momentum_has_no_buffer(lib):
    opt = FusedSGD(_cpu_params(), lr=0.1)
    assert opt.momentum == 0.0 and opt.momentum_buffer is None
    assert opt.state_dict()["momentum_buffer"] is None


# ---------------------------------------------------------------------------------------------------------
# param_groups: one dict, and the attributes are views of it
@pytest.mark.parametrize("cls", [FusedSGD, FusedAdam])
def test_param_groups_and_attributes_agree(lib, cls):
    opt = cls(_cpu_params(), lr=0.1, weight_decay=0.01, max_grad_norm=10.0)
    assert len(opt.param_groups) == 1
    group = opt.param_groups[0]
    extra = {"momentum"} if cls is FusedSGD else {"betas", "eps"}
    assert set(group) == {"params", "lr", "weight_decay", "max_grad_norm"} | extra
    assert all(a is b for a, b in zip(group["params"], opt.params))
    group["lr"] *= 0.1                                            # scripts/train.py:321-323
    assert opt.lr == pytest.approx(0.01)
    opt.lr = 0.5
    assert group["lr"] == 0.5
    for name, value in [("weight_decay", 0.25), ("max_grad_norm", None)] + [
            ("momentum", 0.9)] * (cls is FusedSGD) + [("betas", (0.8, 0.9)), ("eps", 1e-6)] * (cls is FusedAdam):
        group[name] = value
        assert getattr(opt, name) == value
        setattr(opt, name, group[name])
        assert group[name] == value
    assert opt.state_dict()["lr"] == 0.5


# ---------------------------------------------------------------------------------------------------------
# fx_sgd_step: rejected before any HIP call, with a negative status and a message
def test_sgd_step_validation_without_gpu(lib):
    host = torch.zeros(3 * 64)                                    # never dereferenced: every call below returns first
    p, g, buf = (host[i * 64:].data_ptr() for i in range(3))
    ws = host.data_ptr()
    assert p % 16 == 0 and g % 16 == 0 and buf % 16 == 0

    def call(p, g, buf, n, momentum, max_norm, ws):
        return lib.fx_sgd_step(p, g, buf, n, 0.1, momentum, 0.0, max_norm, ws, None, None, None)

    for args, text in [((None, g, None, 8, 0.0, 0.0, None), b"null buffer"),
                       ((p, None, None, 8, 0.0, 0.0, None), b"null buffer"),
                       ((p, g, None, 8, 0.9, 0.0, None), b"momentum needs the momentum buffer"),
                       ((p, g, buf, 8, 0.0, 0.0, None), b"momentum buffer without momentum"),
                       ((p, g, buf, 8, -0.5, 0.0, None), b"momentum must be >= 0"),
                       ((p, g, None, 8, 0.0, 1.0, None), b"clipping needs the grad-norm workspace"),
                       ((p + 4, g, None, 8, 0.0, 0.0, None), b"16-byte aligned"),
                       ((p, g, buf + 8, 8, 0.9, 0.0, None), b"16-byte aligned"),
                       ((p, g, None, -1, 0.0, 0.0, None), b"null buffer")]:
        st = call(*args)
        assert st < 0 and text in lib.fx_last_error(), (args, st, lib.fx_last_error())
    assert call(p, g, None, 0, 0.0, 0.0, None) == 0               # empty problem: nothing to launch
    assert call(p, g, buf, 0, 0.9, 1.0, ws) == 0


def test_sgd_symbol_declared_and_abi_unchanged(lib):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+fx_sgd_step\s*\(([^;{]*?)\)\s*;", src, flags=re.S)
    assert m, "fx_sgd_step is not declared in include/factmx.h"
    assert len(m.group(1).split(",")) == len(nx.SIGNATURES["fx_sgd_step"][1]) == 12
    assert hasattr(ctypes.CDLL(nx.LIB_PATH), "fx_sgd_step")
    assert nx.ABI_VERSION == 30 and lib.fx_version() == 30         # additive: one symbol, no version bump
