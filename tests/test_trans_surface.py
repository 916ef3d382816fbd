"""The transcript-conditioned lockstep path: what is declared, the guard and the pass grouping, the CSR
builder and the host-side argument checks of the two new entry points (CPU)."""
import ctypes
import os

import numpy as np
import pytest

from factmx import functional as fxf
from factmx import native as nx
from factmx.configs import get_cfg_defaults
from factmx.models import blocks, vloss
from factmx.models import blocks_SepVerbNoun as vn
from factmx.models.loss import MatchCriterion

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Seq:
    """Stands for an input tensor on a device this machine may not have."""

    def __init__(self, T, cuda=True):
        self.is_cuda, self.shape = cuda, (T, 40)


def _net(block="iuU", a="sca", match="seq", trans=True, clip=False, a_dim=32):
    cfg = get_cfg_defaults()
    cfg.FACT.update(dict(ntoken=0 if trans else 8, block=block, fpos=True, cmr=0.0, trans=trans))
    cfg.Bi.update(dict(hid_dim=48, dropout=0.0, a=a, a_nhead=4, a_ffdim=48, a_layers=2, a_dim=a_dim,
                       f="m", f_layers=2, f_ln=False, f_dim=24, f_ngp=1))
    cfg.Bu.update(dict(f_layers=2, a_nhead=4))
    cfg.BU.update(dict(f_layers=2, a_nhead=4, s_layers=1))
    cfg.Loss.match = match
    net = (blocks.FACT_CLIP if clip else blocks.FACT)(cfg, 40, 12)
    net.mcriterion = MatchCriterion(cfg, 12, [])
    return net


def test_header_and_binding_declare_the_entries():
    with open(os.path.join(ROOT, "include", "factmx.h")) as fp:
        header = fp.read()
    for name in ("fx_token_embed_fwd", "fx_token_embed_bwd", "fx_eval_pred_trans"):
        assert f"int {name}(" in header and name in nx.SIGNATURES and hasattr(nx.load(), name)
    assert nx.ABI_VERSION >= 27 and f"#define FX_ABI_VERSION {nx.ABI_VERSION}" in header
    assert nx.SIGNATURES["fx_eval_pred_trans"] == nx.SIGNATURES["fx_eval_pred"]


def test_batchable_accepts_transcript_models(monkeypatch):
    assert blocks.TRANS_BATCH is True
    net = _net()
    assert blocks._batchable(net, [_Seq(50)]) and blocks._batchable(net, [_Seq(50), _Seq(7)])
    assert blocks._batchable(net, [_Seq(9)] * 16) and not blocks._batchable(net, [_Seq(9)] * 17)
    assert not blocks._batchable(net, []) and not blocks._batchable(net, [_Seq(50, cuda=False)])
    monkeypatch.setattr(blocks, "TRANS_BATCH", False)
    assert not blocks._batchable(net, [_Seq(50)])
    assert blocks._batchable(_net(trans=False), [_Seq(50)])        # the switch is about transcripts only
    monkeypatch.setattr(blocks, "TRANS_BATCH", True)
    # the GRU input branch (gru / gru_om) has a batched form in the input block of a transcript model
    for a in ("gru", "gru_om"):
        g = _net(block="iU", a=a, match="o2o", a_dim=32 if a == "gru_om" else 48)   # (gru: no output map)
        assert isinstance(g.block_list[0].action_branch, blocks.basic.ActionUpdate_GRU)
        assert blocks._batchable(g, [_Seq(50), _Seq(31)])
        g.cfg.FACT.trans = False
        assert not blocks._batchable(g, [_Seq(50)])
    net.block_list[0].action_branch.layers[0].normalize_before = True          # not a fused-decoder option
    assert not blocks._batchable(net, [_Seq(50)])


def test_pass_grouping():
    tp = blocks.transcript_passes
    assert tp([[2, 5, 9, 2, 5]]) == [[0]]                                   # one video: the shipped config
    assert tp([[2, 5, 9, 2, 5], [1, 2, 3, 4, 5]]) == [[0, 1]]               # equal lengths: one pass
    assert tp([[2, 5, 9, 2, 5], [1, 2, 3, 4, 5], [7, 8, 9, 1]]) == [[0], [1], [2]]   # else one pass per video
    assert tp([[1, 2], [3]]) == [[0], [1]]
    assert tp([[c] * 3 for c in range(17)]) == [list(range(17))] and tp([]) == []
    # 17 videos never reach the grouping: the guard sends them down the per-video path
    assert not blocks._batchable(_net(), [_Seq(9)] * 17)


def test_vloss_supported():
    assert vloss.supported(_net()) and vloss.supported(_net(match="o2o")) and vloss.supported(_net(match="o2m"))
    assert vloss.supported(_net(clip=True)) and vloss.supported(_net(trans=False, match="o2o"))
    assert vloss.supported(_net(block="iU", a="gru_om", match="o2o"))
    assert not vloss.supported(_net(block="i"))                  # no token -> frame attention to match on
    net = _net()
    net.mcriterion = None
    assert not vloss.supported(net)
    net = _net()
    net.cfg.Loss.match = "other"
    assert not vloss.supported(net)


def test_verb_noun_lockstep_still_refuses_transcripts():
    vn.set_verb_noun_ids([0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 0, 2], [0, 1, 2, 3, 4, 5, 6, 0, 1, 2, 3, 6])
    cfg = get_cfg_defaults()
    cfg.FACT.update(dict(ntoken=8, block="IU", fpos=True, cmr=0.0, trans=True))
    cfg.Bi.update(dict(hid_dim=48, dropout=0.0, a="sca", a_nhead=4, a_ffdim=48, a_layers=2, a_dim=32,
                       f="m", f_layers=2, f_ln=False, f_dim=24, f_ngp=1))
    cfg.BU.update(dict(f_layers=2, a_nhead=4, s_layers=1))
    assert not vn._lockstep_ok(vn.FACT(cfg, 40, 5, 7), [_Seq(50)])


def test_token_csr():
    coff, clist = fxf.token_csr([2, 5, 9, 2, 5], 12)
    assert coff.dtype == clist.dtype == np.int32
    np.testing.assert_array_equal(coff, [0, 0, 0, 2, 2, 2, 4, 4, 4, 4, 5, 5, 5])
    np.testing.assert_array_equal(clist, [0, 3, 1, 4, 2])          # each class's rows in increasing order
    coff, clist = fxf.token_csr([3, 3, 3], 4)
    np.testing.assert_array_equal(coff, [0, 0, 0, 0, 3])
    np.testing.assert_array_equal(clist, [0, 1, 2])
    coff, clist = fxf.token_csr([0, 11], 12)
    assert coff[1] == 1 and coff[11] == 1 and coff[12] == 2 and clist.tolist() == [0, 1]
    coff, clist = fxf.token_csr([], 3)
    assert coff.tolist() == [0, 0, 0, 0] and clist.size == 0
    for bad in ([0, 12], [-1, 2]):
        with pytest.raises(ValueError):
            fxf.token_csr(bad, 12)


def _i32(vals):
    return np.asarray(vals, dtype=np.int32)


def test_token_embed_entries_check_their_arguments_on_the_host():
    """Every call below fails on the host: the device pointers (64) are never read, nothing is launched."""
    lib = nx.load()
    ids, pos = _i32([2, 5, 9, 2, 5]), _i32([0, 1, 2, 3, 4])

    def fwd(ids=ids, pos=pos, C=12, A=32, R=5, pe=64, npe=16, ldw=32, ldo=32, ldpe=32, W=64):
        return lib.fx_token_embed_fwd(W, ldw, C, A, ids.ctypes.data, None if pos is None else pos.ctypes.data, 64,
                                      None if pos is None else 64, R, pe, ldpe, npe, 64, ldo, None)
    for kw, text in ((dict(ids=_i32([2, 12, 9, 2, 5])), b"class id out of range"),
                     (dict(ids=_i32([2, -1, 9, 2, 5])), b"class id out of range"),
                     (dict(pos=_i32([0, 1, 2, 3, 16])), b"position out of range"),
                     (dict(pos=None), b"positions without their table"), (dict(W=None), b"bad arguments"),
                     (dict(ldw=31), b"bad arguments"), (dict(ldo=8), b"bad arguments"), (dict(C=0), b"bad arguments"),
                     (dict(ldpe=31), b"positions without their table"), (dict(npe=0), b"positions without their table")):
        assert fwd(**kw) != 0 and text in lib.fx_last_error(), kw
    assert fwd(R=0) == 0                                             # no rows: nothing to do, no launch

    coff, clist = fxf.token_csr(ids, 12)

    def bwd(coff=coff, clist=clist, R=5, C=12, A=32, ldd=32, lddw=32, dW=64):
        return lib.fx_token_embed_bwd(64, ldd, R, C, A, coff.ctypes.data, clist.ctypes.data, 64, 64, dW, lddw, 1, None)
    short = coff.copy()
    short[-1] = 4
    down = coff.copy()
    down[4] = 1
    for kw, text in ((dict(coff=short), b"must cover the R rows"), (dict(coff=down), b"must not decrease"),
                     (dict(clist=_i32([0, 3, 1, 4, 5])), b"row out of range"),
                     (dict(clist=_i32([3, 0, 1, 4, 2])), b"must increase"), (dict(dW=None), b"bad arguments"),
                     (dict(ldd=31), b"bad arguments"), (dict(lddw=31), b"bad arguments"), (dict(R=0), b"bad arguments")):
        assert bwd(**kw) != 0 and text in lib.fx_last_error(), kw


def _video(n=1, **kw):
    arr = nx.array_type(nx.VideoAttn, n)()
    for v in arr:
        v.Q, v.C1, v.T, v.G, v.ldc, v.lda, v.ldf, v.pred_off = 5, 13, 20, 5, 13, 5, 12, 0
        for name in ("clogit", "attn", "seg_id", "flogit", "gs", "ge", "gl"):
            setattr(v, name, 64)           # (never read: every check below fails on the host)
        for k, val in kw.items():
            setattr(v, k, val)
    return arr


def test_eval_pred_trans_checks_every_video_on_the_host():
    lib = nx.load()

    def pred(arr, nvid=1, out=64):
        p = ctypes.addressof(arr)
        return lib.fx_eval_pred_trans(p, p, nvid, 0.1, out, None)
    for bad, text in ((dict(G=6), b"G > Q"), (dict(G=0), b"empty transcript"), (dict(gl=None), b"without a transcript"),
                      (dict(flogit=None), b"without logits"), (dict(C1=1), b"without logits"),
                      (dict(attn=None), b"bad sizes"), (dict(lda=4), b"bad sizes"), (dict(ldf=11), b"bad sizes"),
                      (dict(pred_off=-1), b"bad sizes"), (dict(T=-1), b"bad sizes")):
        assert pred(_video(**bad)) != 0 and text in lib.fx_last_error(), bad
    assert pred(_video(), nvid=0) != 0 and pred(_video(), out=None) != 0
    assert pred(_video(T=0)) == 0                                    # no frames: no launch, no error
    # the second video of a table is checked like the first
    two = _video(2, T=0)
    two[1].G = 9
    assert pred(two, nvid=2) != 0 and b"G > Q" in lib.fx_last_error()
