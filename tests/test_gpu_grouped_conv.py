"""Grouped dilated convolutions (nn.Conv1d(F, F, 3, dilation=d, padding=d, groups=g): the reference's
f_ngp > 1 frame branch) on the GPU against a float64 CPU restatement built on
torch.nn.functional.conv1d(groups=g), applied per video so the zero padding sits at each video's ends:
  * the single layer (fxf.conv3 -> fx_conv3g_fwd / fx_conv3g_bwd): y, dx, dw, db at the smallest shapes that
    cross a 32-row and a 64-row tile edge, a video boundary, an unaligned cg = F / g, depthwise, and a
    dilation larger than the tile; ragged videos through fxf.mstcn(seq_off=);
  * the MSTCN and MSTCN2 stacks with both weight-gradient schedules (plain .grad, FlatGradReducer views)
    and the kernels' dropout mask restated with helpers.drop_mask;
  * a dense MSTCN whose conv weights are the block-diagonal embedding of a grouped module's;
  * bitwise-repeatable weight gradients; ngroup 0 and 1 bitwise the same dense path; one FACT_CLIP step.
Tolerance (tests/test_gpu_mstcn2.py's): max |a - b| <= 2e-4 (1 + max |b|)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as tF

from helpers import drop_mask, drop_subseed
from factmx import functional as fxf

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 2e-4


def _r(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


def _close(a, b, what, tol=TOL):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = (a - b).abs().max().item()
    ref = b.abs().max().item()
    print(f"{what}: max err {err:.3e} (ref max {ref:.3e})")
    assert err <= tol * (1.0 + ref), f"{what}: max err {err:.3e} (ref max {ref:.3e})"


def _offs(T, nvid, seq_off=None):
    return list(seq_off) if seq_off is not None else [v * T for v in range(nvid + 1)]


def _conv(h, w, b, dil, g, offs):
    """rows (N, F) -> Conv1d(k=3, dilation, padding=dilation, groups=g) per video of the row offsets"""
    outs = []
    for v in range(len(offs) - 1):
        hv = h[offs[v]:offs[v + 1]].t().unsqueeze(0)
        outs.append(tF.conv1d(hv, w, b, padding=dil, dilation=dil, groups=g)[0].t())
    return torch.cat(outs, 0)


def _lin(h, w, b):
    return h @ w.reshape(w.shape[0], -1).t() + b


def _masks(seed, n, rows, F, p):
    if p <= 0:
        return [None] * n
    idx = np.arange(rows, dtype=np.int64)[:, None] * F + np.arange(F, dtype=np.int64)[None, :]
    return [torch.from_numpy(drop_mask(drop_subseed(seed, i), idx, p).astype(np.float64)) / (1.0 - float(np.float32(p)))
            for i in range(n)]


def _mstcn_ref(P, x, offs, nl, g, ln, in_map, seed, p):
    """reference basic.py:154-171 / 200-220 with the kernels' dropout mask on every layer's 1x1 branch"""
    h = _lin(x, P["conv_1x1.weight"], P["conv_1x1.bias"]) if in_map else x
    F = h.shape[1]
    masks = _masks(seed, nl, x.shape[0], F, p)
    for i in range(nl):
        q = f"layers.{i}."
        z = torch.relu(_conv(h, P[q + "conv_dilated.weight"], P[q + "conv_dilated.bias"], 2 ** i, g, offs))
        u = _lin(z, P[q + "conv_1x1.weight"], P[q + "conv_1x1.bias"])
        h = h + (u * masks[i] if p > 0 else u)
        if ln:
            h = tF.layer_norm(h, (F,), P[q + "norm.weight"], P[q + "norm.bias"], 1e-5)
    return _lin(h, P["conv_out.weight"], P["conv_out.bias"])


def _mstcn2_ref(P, x, offs, nl, g, seed, p):
    """reference basic.py:263-281 with the kernels' dropout mask on every layer but the last"""
    f = _lin(x, P["conv_1x1_in.weight"], P["conv_1x1_in.bias"])
    F = f.shape[1]
    masks = _masks(seed, nl - 1, x.shape[0], F, p)
    for i in range(nl):
        a = _conv(f, P[f"conv_dilated_1.{i}.weight"], P[f"conv_dilated_1.{i}.bias"], 2 ** (nl - 1 - i), g, offs)
        b = _conv(f, P[f"conv_dilated_2.{i}.weight"], P[f"conv_dilated_2.{i}.bias"], 2 ** i, g, offs)
        r = torch.relu(_lin(torch.cat([a, b], -1), P[f"conv_fusion.{i}.weight"], P[f"conv_fusion.{i}.bias"]))
        if p > 0 and i != nl - 1:
            r = r * masks[i]
        f = f + r
    return _lin(f, P["conv_out.weight"], P["conv_out.bias"])


@pytest.fixture
def seeds(monkeypatch):
    got = []

    def nxt():
        got.append(123456789 + 7919 * len(got))
        return got[-1]
    monkeypatch.setattr(fxf, "dropout_seed", nxt)
    return got


def _params64(mod):
    return {n: t.detach().double().cpu().requires_grad_(True) for n, t in mod.named_parameters()}


def _compare_module(mod, P, xd, xr, y, yr, g, red=None):
    (y * g.float().to(DEV)).sum().backward()
    torch.cuda.synchronize()
    (yr * g).sum().backward()
    _close(y, yr, "y")
    _close(xd.grad, xr.grad, "dx")
    for n, t in mod.named_parameters():
        _close(t.grad, P[n].grad, f"d{n}")
    if red is not None:
        lo = red.flat.data_ptr()
        assert all(lo <= t.grad.data_ptr() < lo + red.flat.numel() * 4 for t in mod.parameters())
    fxf.check_device_status()


# ---------------------------------------------------------------------------------------------------
# 1. the single layer
# ---------------------------------------------------------------------------------------------------
def _conv3_case(F, g, T, nvid, dil, seed=0):
    cg = F // g
    x = _r(T * nvid, F, seed=seed + 1)
    w = _r(F, cg, 3, seed=seed + 2, scale=1.0 / math.sqrt(3 * cg))
    b = _r(F, seed=seed + 3, scale=0.1)
    gy = _r(T * nvid, F, seed=seed + 4)
    xd = x.float().to(DEV).requires_grad_(True)
    wd = w.float().to(DEV).requires_grad_(True)
    bd = b.float().to(DEV).requires_grad_(True)
    y = fxf.conv3(xd, wd, bd, dil, T)
    (y * gy.float().to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return (x, w, b, gy), (xd, wd, bd, y)


@pytest.mark.parametrize("F,g,T,nvid,dil", [(32, 4, 70, 1, 1), (64, 2, 257, 2, 8), (36, 4, 65, 1, 2),
                                             (16, 16, 65, 1, 4), (256, 4, 96, 2, 64)])
def test_conv3_grouped_matches_fp64(F, g, T, nvid, dil):
    (x, w, b, gy), (xd, wd, bd, y) = _conv3_case(F, g, T, nvid, dil)
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
    yr = _conv(xr, wr, br, dil, g, _offs(T, nvid))
    (yr * gy).sum().backward()
    _close(y, yr, "y")
    _close(xd.grad, xr.grad, "dx")
    _close(wd.grad, wr.grad, "dw")
    _close(bd.grad, br.grad, "db")


def test_conv3_grouped_backward_is_bitwise_repeatable():
    _, (_, w1, b1, _) = _conv3_case(64, 2, 257, 2, 8)
    _, (_, w2, b2, _) = _conv3_case(64, 2, 257, 2, 8)
    assert torch.equal(w1.grad, w2.grad) and torch.equal(b1.grad, b2.grad)
    assert w1.grad.abs().max().item() > 0


@pytest.mark.parametrize("flat", [False, True])
def test_grouped_ragged_videos_through_mstcn(flat):
    from factmx.dp import FlatGradReducer
    from factmx.models.basic import MSTCN
    torch.manual_seed(0)
    F, g, nl, offs = 64, 2, 2, [0, 70, 199]
    mod = MSTCN(F, F, 24, nl, dropout=0.0, ln=False, ngroup=g, in_map=False).to(DEV).train()
    red = FlatGradReducer(mod.parameters()) if flat else None
    x, gy = _r(offs[-1], F, seed=1), _r(offs[-1], 24, seed=2)
    xd = x.float().to(DEV).requires_grad_(True)
    y = fxf.mstcn(mod, xd, 0, len(offs) - 1, seq_off=offs)
    P = _params64(mod)
    xr = x.clone().requires_grad_(True)
    yr = _mstcn_ref(P, xr, offs, nl, g, False, False, 0, 0.0)
    _compare_module(mod, P, xd, xr, y, yr, gy, red)


# ---------------------------------------------------------------------------------------------------
# 2. / 3. the stacks
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ln", [True, False])
@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("flat", [False, True])
def test_mstcn_grouped_matches_fp64(ln, p, flat, seeds):
    from factmx.dp import FlatGradReducer
    from factmx.models.basic import MSTCN
    torch.manual_seed(0)
    T, nvid, F, g, nl, cin, cout = 150, 2, 32, 4, 3, 24, 16
    mod = MSTCN(cin, F, cout, nl, dropout=p, ln=ln, ngroup=g, in_map=True).to(DEV).train()
    red = FlatGradReducer(mod.parameters()) if flat else None
    x, gy = _r(T * nvid, cin, seed=1), _r(T * nvid, cout, seed=2)
    xd = x.float().to(DEV).requires_grad_(True)
    y = fxf.mstcn(mod, xd, T, nvid)
    P = _params64(mod)
    xr = x.clone().requires_grad_(True)
    yr = _mstcn_ref(P, xr, _offs(T, nvid), nl, g, ln, True, seeds[-1] if p > 0 else 0, p)
    _compare_module(mod, P, xd, xr, y, yr, gy, red)
    if p > 0:      # eval mode with p > 0 is bitwise the p = 0 path
        mod.eval()
        with torch.no_grad():
            ye = fxf.mstcn(mod, xd, T, nvid)
            mod.dropout_rate = 0.0
            mod.train()
            y0 = fxf.mstcn(mod, xd, T, nvid)
        assert torch.equal(ye, y0)


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("flat", [False, True])
def test_mstcn2_grouped_matches_fp64(p, flat, seeds):
    from factmx.dp import FlatGradReducer
    from factmx.models.basic import MSTCN2
    torch.manual_seed(0)
    T, nvid, F, g, nl, cin, cout = 200, 2, 64, 2, 4, 48, 24
    mod = MSTCN2(cin, F, cout, nl, dropout=p, ngroup=g, in_map=True).to(DEV).train()
    red = FlatGradReducer(mod.parameters()) if flat else None
    x, gy = _r(T * nvid, cin, seed=1), _r(T * nvid, cout, seed=2)
    xd = x.float().to(DEV).requires_grad_(True)
    y = mod(xd, T)[:, 0]
    P = _params64(mod)
    xr = x.clone().requires_grad_(True)
    yr = _mstcn2_ref(P, xr, _offs(T, nvid), nl, g, seeds[-1] if p > 0 else 0, p)
    _compare_module(mod, P, xd, xr, y, yr, gy, red)
    if p > 0:
        mod.eval()
        with torch.no_grad():
            ye = mod(xd, T)
            mod.dropout.p = 0.0
            mod.train()
            y0 = mod(xd, T)
        assert torch.equal(ye, y0)


# ---------------------------------------------------------------------------------------------------
# 4. against the dense path
# ---------------------------------------------------------------------------------------------------
def test_grouped_equals_block_diagonal_dense():
    from factmx.models.basic import MSTCN
    torch.manual_seed(0)
    T, nvid, F, g, nl = 130, 2, 64, 4, 3
    cg = F // g
    grp = MSTCN(F, F, 24, nl, dropout=0.0, ln=False, ngroup=g, in_map=False).to(DEV).train()
    dense = MSTCN(F, F, 24, nl, dropout=0.0, ln=False, ngroup=1, in_map=False).to(DEV).train()
    sd = {k: v.clone() for k, v in grp.state_dict().items()}
    for i in range(nl):
        w = sd[f"layers.{i}.conv_dilated.weight"]
        wd = torch.zeros(F, F, 3, device=DEV)
        for q in range(g):
            wd[q * cg:(q + 1) * cg, q * cg:(q + 1) * cg] = w[q * cg:(q + 1) * cg]
        sd[f"layers.{i}.conv_dilated.weight"] = wd
    dense.load_state_dict(sd, strict=True)
    x, gy = _r(T * nvid, F, seed=1).float().to(DEV), _r(T * nvid, 24, seed=2).float().to(DEV)
    res = []
    for mod in (grp, dense):
        xd = x.clone().requires_grad_(True)
        y = fxf.mstcn(mod, xd, T, nvid)
        (y * gy).sum().backward()
        torch.cuda.synchronize()
        res.append((y, xd.grad))
    _close(res[0][0], res[1][0], "y vs dense")
    _close(res[0][1], res[1][1], "dx vs dense")
    gp, dp = dict(grp.named_parameters()), dict(dense.named_parameters())
    for n in gp:
        if n.endswith("conv_dilated.weight"):
            blocks = torch.cat([dp[n].grad[q * cg:(q + 1) * cg, q * cg:(q + 1) * cg] for q in range(g)], 0)
            _close(gp[n].grad, blocks, f"d{n} vs dense diagonal blocks")
        else:
            _close(gp[n].grad, dp[n].grad, f"d{n} vs dense")
    fxf.check_device_status()


# ---------------------------------------------------------------------------------------------------
# 6. ngroup 0 / 1: the dense path, untouched
# ---------------------------------------------------------------------------------------------------
def test_ngroup_zero_and_one_are_the_same_dense_path():
    from factmx.models.basic import MSTCN, MSTCN2
    torch.manual_seed(0)
    T, nvid, F = 130, 2, 64
    x = _r(T * nvid, F, seed=1).float().to(DEV)
    for mod in (MSTCN(F, F, 24, 3, dropout=0.0, ln=True, in_map=False), MSTCN(F, F, 24, 3, dropout=0.0, ln=False),
                MSTCN2(F, F, 24, 3, dropout=0.0, in_map=True)):
        mod = mod.to(DEV).train()
        outs = []
        for ng in (1, 0):
            mod.ngroup = ng     # -> fx_mstcn_params.ngroup / fx_mstcn2_params.ngroup
            mod.zero_grad(set_to_none=True)
            xd = x.clone().requires_grad_(True)
            y = fxf.mstcn(mod, xd, T, nvid) if isinstance(mod, MSTCN) else mod(xd, T)
            y.sum().backward()
            torch.cuda.synchronize()
            outs.append([y.detach().clone(), xd.grad.clone()] + [p.grad.clone() for p in mod.parameters()])
        assert all(torch.equal(a, b) for a, b in zip(*outs))
    # the dense single layer (g = 1) still is the implicit-GEMM path: same bits on a second run
    (x64, w, b, gy), (xd, wd, bd, y) = _conv3_case(32, 1, 70, 1, 2)
    _, (xd2, wd2, bd2, y2) = _conv3_case(32, 1, 70, 1, 2)
    assert torch.equal(y, y2) and torch.equal(xd.grad, xd2.grad)
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x64, w, b))
    _close(y, _conv(xr, wr, br, 2, 1, [0, 70]), "dense conv3 y")


# ---------------------------------------------------------------------------------------------------
# 7. model level
# ---------------------------------------------------------------------------------------------------
def test_fact_clip_trains_with_grouped_frame_branch():
    from helpers import load_fixture, tiny_meta, cfg_from_meta, tiny_inputs
    import paramgen as pg
    from factmx.models.blocks import FACT_CLIP
    from factmx.models.loss import MatchCriterion
    meta = tiny_meta(load_fixture("tiny_clip"))
    cfg = cfg_from_meta(meta)
    cfg.Bi.f_ngp = 2
    C, D = meta["C"], meta["D"]
    feats, label, text = tiny_inputs(meta)
    torch.manual_seed(123)
    net = FACT_CLIP(cfg, D, C, text_embeddings=torch.from_numpy(text).float())
    with torch.no_grad():
        for n, p in net.named_parameters():
            p.copy_(torch.from_numpy(pg.param_value(n, p.shape, meta["seed"])))
    assert any(p.shape[1] * 2 == p.shape[0] for n, p in net.named_parameters() if n.endswith("conv_dilated.weight"))
    net.mcriterion = MatchCriterion(cfg, C, [])
    net = net.to(DEV).train()
    loss, _ = net([torch.from_numpy(feats).float().to(DEV)], [torch.from_numpy(label).to(DEV)], compute_loss=True)
    loss.backward()
    torch.cuda.synchronize()
    assert math.isfinite(loss.item())
    for n, p in net.named_parameters():
        assert p.grad is not None, n
        assert torch.isfinite(p.grad).all(), n
        assert p.grad.abs().max().item() > 0, n
    fxf.check_device_status()
