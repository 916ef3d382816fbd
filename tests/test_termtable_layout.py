"""The term table builder's layout (models/termtable.TermTable) and the verb/noun table's source records
(models/vn_vloss._sources / _batch_sources / _fill) on plain CPU tensors, up to but not including ``send``:
no device, no native library (CPU)."""
import ctypes
import itertools
import types

import numpy as np
import pytest
import torch

from factmx import functional as fxf
from factmx import native as nx
from factmx.models import vn_vloss
from factmx.models.termtable import TermTable, _Pack

KCAP = 3


def _table():
    """A class term on rows 0..4 and a VNCLASS term on rows 5.. of one shared (12, 6) input, an ATTN term of
    each axis on its own logits, the shared input registered twice."""
    X = torch.randn(12, 6)
    Lf, La = torch.randn(4, 9), torch.randn(9, 4)          # (Q, S) read as (S, Q); (S, Q)
    pk = _Pack()
    pk.array(np.arange(5), np.int32)                       # (something of the caller's reserved first)
    tt = TermTable(pk, "cpu", [X, Lf, X, La], np.zeros((2, 4), dtype=np.float32), nvn=1)
    specs = [(nx.TERM_CLASS, 5, 6, X, 0, 6, 1, 6, 1, 0),
             (nx.TERM_VNCLASS, 7, 6, X, 5 * 6, 6, 1, 6, 1, 0),
             (nx.TERM_ATTN, 9, 4, Lf, 0, 1, 9, 1, 9, KCAP),
             (nx.TERM_ATTN, 9, 4, La, 0, 4, 1, 4, 1, KCAP)]
    for kind, R, C, g, off, sr, sc, dsr, dsc, kcap in specs:
        t = tt.add(kind, R, C, g.data_ptr() + 4 * off, sr, sc, g, off, dsr, dsc, 0.5, 0.0, kcap)
        assert t.slot == len(tt._slots) - 1
    tt.lay_out()
    return tt, pk, (X, Lf, La), specs


def test_arena_one_aligned_slice_per_input():
    tt, _, (X, Lf, La), specs = _table()
    assert [id(t) for t in tt.inputs] == [id(X), id(Lf), id(La)]           # first seen first, X once
    spans = []
    for t, off, (shape, strides) in zip(tt.inputs, *tt.grads()):
        assert (4 * off) % 256 == 0
        assert tt.grad_ptr(t) == tt.gflat.data_ptr() + 4 * off
        g = tt.gflat.as_strided(shape, strides, off)                       # what the backward hands out
        assert g.shape == t.shape and g.is_contiguous() and g.data_ptr() == tt.grad_ptr(t)
        assert tt.grad_slice(t).data_ptr() == tt.grad_ptr(t) and tt.grad_slice(t).numel() == t.numel()
        spans.append((off, off + t.numel()))
    for (a0, a1), (b0, b1) in itertools.combinations(spans, 2):
        assert a1 <= b0 or b1 <= a0
    assert max(s[1] for s in spans) <= tt.gflat.numel()
    for i, (kind, R, C, g, off, *_rest) in enumerate(specs):
        assert tt.terms[i].dx == tt.grad_ptr(g) + 4 * off == tt.grad_ptr(g, off)


def test_terms_scratch_and_coefficients():
    tt, pk, _, specs = _table()
    assert tt.nterms == len(tt.terms) == 4 and tt.coef.shape == (tt.nout, tt.nterms) == (2, 4)
    assert tt.scr.numel() >= 1
    lo, hi = tt.scr.data_ptr(), tt.scr.data_ptr() + 4 * tt.scr.numel()
    spans = []
    for i, (kind, R, C, *_rest) in enumerate(specs):
        t = tt.terms[i]
        assert (t.slot, t.kind, t.R, t.C) == (i, kind, R, C)
        want = {nx.TERM_CLASS: (R, 0, 0), nx.TERM_VNCLASS: (2 * R, 0, 0), nx.TERM_ATTN: (R, R + KCAP, KCAP)}[kind]
        assert tt._slots[i] == want
        for p, n in zip((t.lse, t.lse2, t.colz), want):
            assert p % 16 == 0 and lo <= p and p + 4 * n <= hi
            spans.append((p, p + 4 * max(n, 1)))
    for (a0, a1), (b0, b1) in itertools.combinations(spans, 2):
        assert a1 <= b0 or b1 <= a0
    # an InfoNCE term's slots: rows, classes, the caller's column scratch
    tt2 = TermTable(_Pack(), "cpu", [torch.zeros(3, 2)], np.zeros((1, 1), dtype=np.float32))
    tt2.add(nx.TERM_INFONCE, 3, 5, 0, 5, 1, None, 0, 5, 1, 0.5, 0.0, 0, 77)
    assert tt2._slots == [(3, 5, 77)] and tt2.terms[0].dx is None
    # the structs and the coefficients stay writable until send: what the pack sends is what was written last
    tt.terms[0].c_ce = 0.125
    tt.terms[2].K = 2
    tt.coef[1, 3] = 7.0
    sent = [a for _, a in pk.items if isinstance(a, ctypes.Array) and a._type_ is nx.LossTerm]
    assert len(sent) == 1 and sent[0] is tt.terms
    assert sent[0][0].c_ce == 0.125 and sent[0][2].K == 2
    assert any(isinstance(a, np.ndarray) and np.shares_memory(a, tt.coef) for _, a in pk.items)


def test_empty_table_still_has_scratch():
    tt = TermTable(_Pack(), "cpu", [], np.zeros((1, 0), dtype=np.float32))
    tt.lay_out()
    assert tt.scr.numel() >= 1


def test_single_mapping_fill():
    tt, _, _, _ = _table()
    m = fxf.VerbNounMap([0, 1, 1, 0], [0, 1, 2, 3])
    dev_addr, host_addr = tt.vn(0, m, 1)
    v = tt.vnt[0]
    assert (v.n1, v.n2, v.A, v.null) == (3, 5, 4, 1) and host_addr == ctypes.addressof(v)
    assert dev_addr == tt.base + tt._o_vn
    assert (v.vids, v.nids) == tuple(t.data_ptr() for t in m.tables("cpu"))
    assert (v.voff, v.vlist, v.noff, v.nlist) == tuple(t.data_ptr() for t in m.csr("cpu", 3, 5))


# ---------------------------------------------------------------------------
# the verb/noun table: one video's blocks against the same rows of the stacked batch tensors
# ---------------------------------------------------------------------------

Q, V, N = 4, 2, 3
TS, SEGS, KINDS = [7, 5], [[3, 2], [4, 3]], ["I", "U"]           # SEGS[block][video]
FIELDS = ("kind", "R", "C", "axis", "K", "sr", "sc", "dsr", "dsc", "c_ce", "c_sm", "D")


def _batch():
    fo = [0, 7, 12]
    bts = []
    for S in SEGS:
        s_off = [0, S[0], S[0] + S[1]]
        local = [(torch.zeros(T, dtype=torch.int32), torch.zeros(Sv, dtype=torch.int32),
                  torch.zeros(Sv, dtype=torch.int32)) for T, Sv in zip(TS, S)]
        bts.append(dict(f_cl=torch.randn(fo[-1], V + N), seg_cl=torch.randn(s_off[-1], V + N),
                        a_cl=torch.randn(len(TS) * Q, V + N + 2), f2a_lg=torch.randn(Q * s_off[-1]),
                        a2f_lg=torch.randn(Q * s_off[-1]), S=S, s_off=s_off, local=local))
    return bts, fo


def _video_blocks(bts, fo, v):
    """Stand-in blocks of video v alone: views of the stacked tensors' rows, shaped as the per-video path
    keeps them."""
    blocks = []
    for bt in bts:
        Sv, s0 = bt["S"][v], bt["s_off"][v]
        lg = slice(Q * s0, Q * (s0 + Sv))
        blocks.append(types.SimpleNamespace(
            _clogits=(bt["f_cl"][fo[v]:fo[v + 1]].unsqueeze(1), bt["seg_cl"][s0:s0 + Sv].unsqueeze(1),
                      bt["a_cl"][v * Q:(v + 1) * Q].unsqueeze(1)),
            f2a_attn_logit=bt["f2a_lg"][lg].view(1, Q, Sv), a2f_attn_logit=bt["a2f_lg"][lg].view(1, Sv, Q),
            tdu=types.SimpleNamespace(start32=bt["local"][v][1], end32=bt["local"][v][2], num_seg=Sv)))
    return blocks


def _filled(rows, coef, src, vids):
    tt = TermTable(_Pack(), "cpu", vn_vloss._inputs(src), coef, nvn=2)
    m = fxf.VerbNounMap([0, 1, 1, 0], [0, 1, 2, 2])
    vn_vloss._fill(tt, rows, src, vids, 4096, tt.vn_pair(m))
    return tt


def _vid(v):
    return vn_vloss._Vid(TS[v], 2 + v, 1000 + v, 2000 + v, [3000 + v, 3100 + v, 3200 + v, 3300 + v])


def _rel(tt, rows, src):
    """Per term: the non-address fields, and the x / dx offsets relative to the storage they point into."""
    out = []
    for t, (v, k, name, _, _) in zip(tt.terms, rows):
        s = getattr(src[v][k], name)
        out.append((tuple(getattr(t, f) for f in FIELDS), t.x - s.x.data_ptr(), t.dx - tt.grad_ptr(s.t),
                    (t.y, t.w, t.rs, t.re, t.ka, t.kgs, t.kge, t.ksw), t.vn == tt.base + tt._o_vn))
    return out


def test_single_video_sources_equal_the_batch_of_one():
    bts, fo = _batch()
    one = [dict(bt, f_cl=bt["f_cl"][:7], seg_cl=bt["seg_cl"][:bt["S"][0]], a_cl=bt["a_cl"][:Q],
                f2a_lg=bt["f2a_lg"][:Q * bt["S"][0]], a2f_lg=bt["a2f_lg"][:Q * bt["S"][0]], S=bt["S"][:1],
                s_off=bt["s_off"][:2], local=bt["local"][:1]) for bt in bts]
    S0 = [S[0] for S in SEGS]
    rows, coef = vn_vloss.term_plan(KINDS, TS[0], S0, Q, 4, 0.3)
    rows = [(0,) + r for r in rows]
    src_a = vn_vloss._sources(_video_blocks(bts, fo, 0), KINDS, S0, Q)
    src_b = vn_vloss._batch_sources(one, KINDS, TS[:1], fo[:2], Q)
    ta, tb = _filled(rows, coef, src_a, [_vid(0)]), _filled(rows, coef.copy(), src_b, [_vid(0)])
    assert len(rows) == 3 + 5 and ta.nterms == tb.nterms == len(rows)
    assert _rel(ta, rows, src_a) == _rel(tb, rows, src_b)
    assert all(off_x == 0 and off_dx == 0 for _, off_x, off_dx, _, _ in _rel(tb, rows, src_b))


def test_batch_rows_sit_at_each_videos_offsets():
    """Every term of video v in the batch table reads the very rows video v's own blocks hold, and its
    gradient sits at the same element offset of the stacked input's slice."""
    bts, fo = _batch()
    rows, coef = vn_vloss.batch_plan(KINDS, TS, SEGS, Q, 4, 0.3)
    src = vn_vloss._batch_sources(bts, KINDS, TS, fo, Q)
    tb = _filled(rows, coef, src, [_vid(0), _vid(1)])
    assert [t.slot for t in tb.terms] == list(range(len(rows)))
    i = 0
    for v in range(2):
        blocks = _video_blocks(bts, fo, v)
        r1, c1 = vn_vloss.term_plan(KINDS, TS[v], [S[v] for S in SEGS], Q, 4, 0.3)
        r1 = [(0,) + r for r in r1]
        src1 = vn_vloss._sources(blocks, KINDS, [S[v] for S in SEGS], Q)
        t1 = _filled(r1, c1, src1, [_vid(v)])
        for a, (_, k, name, _, _) in zip(t1.terms, r1):
            b = tb.terms[i]
            assert tuple(getattr(a, f) for f in FIELDS) == tuple(getattr(b, f) for f in FIELDS), (v, k, name)
            assert a.x == b.x, (v, k, name)                        # the same storage: absolute addresses agree
            s1, sb = getattr(src1[0][k], name), getattr(src[v][k], name)
            row0 = s1.t.storage_offset() - sb.t.storage_offset()   # (contiguous stacks: elements = gradient offset)
            assert b.dx == tb.grad_ptr(sb.t) + 4 * row0 and a.dx == t1.grad_ptr(s1.t), (v, k, name)
            assert (a.y, a.rs, a.re, a.ka) == (b.y, b.rs, b.re, b.ka)
            i += 1
    assert i == len(rows)


def test_a_wrong_row_offset_shows():
    bts, fo = _batch()
    rows, coef = vn_vloss.batch_plan(KINDS, TS, SEGS, Q, 4, 0.3)
    good = vn_vloss._batch_sources(bts, KINDS, TS, fo, Q)
    bad = vn_vloss._batch_sources(bts, KINDS, TS, [0, 6, 12], Q)             # video 1 one frame row early
    tg, tb = _filled(rows, coef, good, [_vid(0), _vid(1)]), _filled(rows, coef.copy(), bad, [_vid(0), _vid(1)])
    moved = [(v, name) for (v, _, name, _, _), a, b in zip(rows, tg.terms, tb.terms) if a.x != b.x]
    assert moved == [(1, "frame"), (1, "frame")]


def test_attention_logits_of_another_shape_are_refused():
    bts, fo = _batch()
    blocks = _video_blocks(bts, fo, 1)                   # (3 segments x 4 tokens in the update block)
    blocks[1].a2f_attn_logit = blocks[1].a2f_attn_logit.transpose(1, 2)
    with pytest.raises(RuntimeError):
        vn_vloss._sources(blocks, KINDS, [S[1] for S in SEGS], Q)
    bts[1]["f2a_lg"] = bts[1]["f2a_lg"][:-1]
    with pytest.raises(RuntimeError):
        vn_vloss._batch_sources(bts, KINDS, TS, fo, Q)
