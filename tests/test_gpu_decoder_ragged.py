"""Videos with different token counts in one fused decoder call (fx_decoder_params.tok_off, GPU).

A stacked call whose videos own token rows tok_off[v]:tok_off[v+1] (and memory rows mem_off[v]:mem_off[v+1])
against the float64 oracle fo.sca_decoder / fo.sa_decoder run per video and concatenated, the same gout
rows, parameter gradients summed over the videos; tolerances of tests/test_gpu_decoder.py (out 2e-5, input
gradients 1e-4, parameter gradients 2e-4 of the reference maximum).  The shapes are the smallest that reach
each attention core's edge:

* the LDS-resident small attention (attn_small.hip): a one-token video, a 64-token one;
* the persistent token kernel (tokdec.hip): 32 / 1 / 17 tokens, fx_prof kind 8 proves it ran;
* more than 64 tokens (attn_t_lds.hip in query blocks of 64): 70 and 3 tokens -- the second query block has
  no query of the short video -- at head dim 8 and 32;
* the register-resident head-dim-32 cross attention with ragged queries and ragged memory;
* tok_off of an even split is bitwise tok_off = None; dropout masks are indexed by global stacked rows
  (the masked float64 restatement of tests/test_gpu_decoder_ext.py), the backward redraws the forward's;
* bad offsets are refused.
"""
import ctypes

import numpy as np
import pytest
import torch

from factmx import functional as fxf
from factmx import native as nx
from factmx.models import basic
from oracle import fact_oracle as fo
from test_gpu_decoder import _close, _seed_params
from test_gpu_decoder_ext import _Masks, _mha_masked, _tok_launches
from test_gpu_decoder_ext import _close as _close_abs

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _build(cross, A, h, FF, Hm, L, p=0.0):
    if cross:
        layer = basic.SCALayer(A, Hm, h, FF, dropout=p, attn_dropout=p)
        dec = basic.SCADecoder(A, A, 2 * A, layer, L, norm=torch.nn.LayerNorm(A), in_map=False)
    else:
        layer = basic.SALayer(A, h, dim_feedforward=FF, dropout=p, attn_dropout=p)
        dec = basic.SADecoder(A, A, 2 * A, layer, L, in_map=False)
    _seed_params(dec, 1)
    return dec.to(DEV).train()


def _inputs(cross, counts, mems, A, Hm, use_qpos, use_pos):
    g = torch.Generator().manual_seed(2)
    R = sum(counts)
    T = sum(mems) if cross else 0
    t = {"tgt": torch.randn(R, A, generator=g, dtype=torch.float64),
         "qpos": torch.randn(R, A, generator=g, dtype=torch.float64) if use_qpos else None,
         "mem": torch.randn(T, Hm, generator=g, dtype=torch.float64) if cross else None,
         "pos": torch.randn(T, Hm, generator=g, dtype=torch.float64) if (cross and use_pos) else None,
         "gout": torch.randn(R, 2 * A, generator=g, dtype=torch.float64)}
    return t


def _off(counts):
    return [0] + [int(x) for x in np.cumsum(counts)]


def _gpu_run(dec, t, nvid, mem_off, tok_off):
    d = {k: (None if v is None else v.float().to(DEV).requires_grad_(k != "gout")) for k, v in t.items()}
    for p in dec.parameters():
        p.grad = None
    y = fxf.decoder(dec, d["tgt"], d["mem"], pos=d["pos"], query_pos=d["qpos"], nvid=nvid, mem_off=mem_off,
                    tok_off=tok_off)
    (y * d["gout"]).sum().backward()
    fxf.side_join()
    torch.cuda.synchronize()
    fxf.check_device_status()
    grads = {k: d[k].grad for k in ("tgt", "qpos", "mem", "pos") if d[k] is not None}
    return y.detach(), grads, {n: p.grad.clone() for n, p in dec.named_parameters()}


def _oracle(dec, cross, t, counts, mems, L, h):
    P = {n: p.detach().double().cpu().requires_grad_(True) for n, p in dec.named_parameters()}
    r = {k: (None if v is None else v.clone().requires_grad_(k != "gout")) for k, v in t.items()}
    to, mo = _off(counts), _off(mems) if cross else None
    outs = []
    for v in range(len(counts)):
        rs = slice(to[v], to[v + 1])
        qp = None if r["qpos"] is None else r["qpos"][rs]
        if cross:
            ms = slice(mo[v], mo[v + 1])
            outs.append(fo.sca_decoder(P, "", r["tgt"][rs], r["mem"][ms], None if r["pos"] is None else r["pos"][ms],
                                       qp, L, h))
        else:
            outs.append(fo.sa_decoder(P, "", r["tgt"][rs], qp, L, h))
    ref = torch.cat(outs)
    (ref * r["gout"]).sum().backward()
    return ref.detach(), {k: r[k].grad for k in ("tgt", "qpos", "mem", "pos") if r[k] is not None}, \
        {n: P[n].grad for n in P}


def _case(cross, counts, mems, A, h, FF, Hm, L, use_qpos=True, use_pos=True, expect_tok=None):
    dec = _build(cross, A, h, FF, Hm, L)
    assert basic._fused_decoder_ok(dec)
    t = _inputs(cross, counts, mems, A, Hm, use_qpos, use_pos)
    lib = nx.load()
    assert lib.fx_prof_enable(8, 64) == 0
    try:
        y, gi, gp = _gpu_run(dec, t, len(counts), _off(mems) if cross else None, _off(counts))
        ntok = _tok_launches(lib)
    finally:
        lib.fx_prof_disable()
    if expect_tok is not None:
        assert (ntok > 0) == expect_tok, ntok
    assert int(fxf.device_status(torch.device(DEV, torch.cuda.current_device()))[0]) == 0
    ref, ri, rp = _oracle(dec, cross, t, counts, mems, L, h)
    _close(y, ref, 2e-5, "out")
    for k in gi:
        _close(gi[k], ri[k], 1e-4, f"d {k}")
    for n in gp:
        _close(gp[n], rp[n], 2e-4, f"d {n}")


@pytest.mark.parametrize("use_qpos", [True, False])
def test_small_attention_cross_decoder(use_qpos):
    _case(True, [5, 4, 1], [77, 200, 33], 32, 4, 64, 64, 2, use_qpos=use_qpos, expect_tok=False)


def test_small_attention_sa_decoder():
    _case(False, [8, 1, 64], None, 32, 4, 64, 0, 3, expect_tok=False)


def test_token_kernel():
    _case(True, [32, 1, 17], [256, 130, 64], 256, 8, 512, 512, 2, expect_tok=True)


def test_token_kernel_sa_decoder():
    _case(False, [17, 32, 1], None, 128, 4, 192, 0, 2, expect_tok=True)


@pytest.mark.parametrize("A,h", [(48, 6), (64, 2)])
def test_over_64_tokens_empty_query_block(A, h):
    """70 and 3 tokens: the second query block of 64 holds no query of video 1 (its workgroups and its
    merge workgroup leave at once; the dK / dV of video 1 come from the first block alone)."""
    _case(False, [70, 3], None, A, h, 96, 0, 2, expect_tok=False)


def test_over_64_tokens_cross_decoder():
    """The cross attention in query blocks too: video 1 has no query in the second block."""
    _case(True, [70, 3], [100, 37], 64, 2, 96, 80, 2, expect_tok=False)


def test_register_resident_cross_attention():
    _case(True, [32, 1, 5], [300, 64, 65], 128, 4, 256, 96, 2)


@pytest.mark.parametrize("Q,A,h,FF,Hm", [(5, 32, 4, 64, 64), (17, 256, 8, 512, 512)])
def test_even_offsets_are_bitwise_the_even_split(Q, A, h, FF, Hm):
    dec = _build(True, A, h, FF, Hm, 2)
    t = _inputs(True, [Q, Q], [90, 90], A, Hm, True, True)
    y0, gi0, gp0 = _gpu_run(dec, t, 2, None, None)
    y1, gi1, gp1 = _gpu_run(dec, t, 2, None, [0, Q, 2 * Q])
    assert torch.equal(y0, y1)
    for k in gi0:
        assert torch.equal(gi0[k], gi1[k]), k
    for n in gp0:
        assert torch.equal(gp0[n], gp1[n]), n


def _ref_masked(P, tgt, qpos, mem, mpos, to, mo, nl, nh, M):
    """tests/test_gpu_decoder_ext.py _ref_decoder (SCADecoder, dropout from _Masks) over videos of token rows
    to[v]:to[v+1]: every mask indexed by the global stacked rows."""
    nvid, A, R = len(to) - 1, tgt.shape[1], tgt.shape[0]
    x = tgt
    for l in range(nl):
        p = f"layers.{l}."
        outs = []
        for v in range(nvid):
            r = slice(to[v], to[v + 1])
            rows = np.arange(to[v], to[v + 1])
            q = fo.add_pos(x[r], qpos[r])
            outs.append(_mha_masked(P, p + "self_attn.", q, q, x[r], nh, M.probs(l, 0, rows, rows, R)))
        t = fo.layer_norm(x + torch.cat(outs) * M.branch(l, 1, A), P[p + "norm1.weight"], P[p + "norm1.bias"])
        outs = []
        for v in range(nvid):
            r, m = slice(to[v], to[v + 1]), slice(mo[v], mo[v + 1])
            keep = M.probs(l, 2, np.arange(to[v], to[v + 1]), np.arange(mo[v], mo[v + 1]), mo[-1])
            outs.append(_mha_masked(P, p + "multihead_attn.", fo.add_pos(t[r], qpos[r]), fo.add_pos(mem[m], mpos[m]),
                                    mem[m], nh, keep))
        t = fo.layer_norm(t + torch.cat(outs) * M.branch(l, 3, A), P[p + "norm2.weight"], P[p + "norm2.bias"])
        FF = P[p + "linear1.weight"].shape[0]
        hid = torch.relu(fo.linear(t, P[p + "linear1.weight"], P[p + "linear1.bias"])) * M.branch(l, 4, FF)
        ff = fo.linear(hid, P[p + "linear2.weight"], P[p + "linear2.bias"]) * M.branch(l, 5, A)
        x = fo.layer_norm(t + ff, P[p + "norm3.weight"], P[p + "norm3.bias"])
    x = fo.layer_norm(x, P["norm.weight"], P["norm.bias"])
    return fo.linear(x, P["out_linear.weight"], P["out_linear.bias"])


def test_dropout_masks_use_global_rows(monkeypatch):
    """dropout = attn_dropout = 0.2 on counts [5, 4, 1]: two runs with one seed are bitwise equal, and output
    and gradients match the float64 restatement under the documented masks (so the backward redrew the
    forward's); tolerances of tests/test_gpu_decoder_ext.py."""
    seed = 0x5DEECE66D * 3 % 2 ** 62
    monkeypatch.setattr(fxf, "dropout_seed", lambda: seed)
    counts, mems, A, h, L, p = [5, 4, 1], [77, 200, 33], 32, 4, 2, 0.2
    dec = _build(True, A, h, 64, 64, L, p)
    t = _inputs(True, counts, mems, A, 64, True, True)
    to, mo = _off(counts), _off(mems)
    y, gi, gp = _gpu_run(dec, t, 3, mo, to)
    y2, gi2, gp2 = _gpu_run(dec, t, 3, mo, to)
    assert torch.equal(y, y2)
    for k in gi:
        assert torch.equal(gi[k], gi2[k]), k
    for n in gp:
        assert torch.equal(gp[n], gp2[n]), n
    M = _Masks(seed, p, p, sum(counts), h)
    P = {n: q.detach().double().cpu().requires_grad_(True) for n, q in dec.named_parameters()}
    r = {k: v.clone().requires_grad_(k != "gout") for k, v in t.items()}
    yr = _ref_masked(P, r["tgt"], r["qpos"], r["mem"], r["pos"], to, mo, L, h, M)
    (yr * r["gout"]).sum().backward()
    _close_abs(y, yr, rtol=2e-4, atol=2e-4, what="out")
    for k in gi:
        _close_abs(gi[k], r[k].grad, rtol=2e-4, atol=2e-4, what=f"d {k}")
    for n in gp:
        _close_abs(gp[n], P[n].grad, rtol=5e-4, atol=5e-4, what=f"d {n}")


@pytest.mark.parametrize("tok_off", [[0, 6, 4, 10], [0, 5, 9, 11], [0, 5, 5, 10]],
                         ids=["not_increasing", "end_not_R", "empty_video"])
def test_bad_offsets_are_refused(tok_off):
    dec = _build(False, 32, 4, 64, 0, 1)
    x = torch.randn(10, 32, device=DEV)
    with pytest.raises(nx.FactmxNativeError):
        fxf.decoder(dec, x, None, query_pos=None, nvid=3, tok_off=tok_off)
    torch.cuda.synchronize()
    y = fxf.decoder(dec, x, None, query_pos=None, nvid=3, tok_off=[0, 5, 9, 10])   # (and the device is fine)
    assert torch.isfinite(y).all()
