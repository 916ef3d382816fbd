"""The verb/noun model's lockstep step: what is declared, its switch and guard, the host-side argument
checks of the batched entries and the batch coefficient matrix (CPU)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from factmx import native as nx
from factmx.configs import get_cfg_defaults
from factmx.models import blocks
from factmx.models import blocks_SepVerbNoun as vn
from factmx.models import vn_vloss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIELDS = ["Q", "T", "G", "nattn", "action_clogit", "lda", "frame_clogit", "ldf", "attn", "ldattn", "seg_id",
          "seg_start", "seg_end", "gs", "ge", "gl", "pred_off"]


def test_header_and_binding_declare_the_batched_entries():
    with open(os.path.join(ROOT, "include", "factmx.h")) as fp:
        header = fp.read()
    assert "int fx_vn_match_cost_batch(" in header and "int fx_vn_eval_pred_batch(" in header
    body = re.search(r"typedef struct fx_vn_video\s*\{(.*?)\}\s*fx_vn_video\s*;", header, flags=re.S).group(1)
    names = []
    for stmt in body.split(";"):
        names += re.findall(r"(\w+)\s*(?:,|$)", stmt.strip())
    assert names == FIELDS == [f[0] for f in nx.VnVideo._fields_]
    assert "fx_vn_match_cost_batch" in nx.SIGNATURES and "fx_vn_eval_pred_batch" in nx.SIGNATURES
    assert nx.VnVideo in nx.ABI_STRUCTS and nx.ABI_STRUCTS.index(nx.VnVideo) == 7
    assert nx.ABI_VERSION >= 26 and f"#define FX_ABI_VERSION {nx.ABI_VERSION}" in header
    assert nx.load().fx_struct_size(7) == ctypes.sizeof(nx.VnVideo)


def _video(**kw):
    arr = nx.array_type(nx.VnVideo, 1)()
    v = arr[0]
    v.Q, v.T, v.G, v.nattn, v.lda, v.ldf, v.ldattn = 8, 20, 3, 5, 14, 12, 8
    # (never read: every check below fails on the host, before any pointer is used)
    for name in ("action_clogit", "frame_clogit", "attn", "seg_id", "seg_start", "seg_end", "gs", "ge", "gl"):
        setattr(v, name, 64)
    for k, val in kw.items():
        setattr(v, k, val)
    return arr


def test_batched_entries_check_every_video_on_the_host():
    lib = nx.load()

    def cost(arr, n1=5, n2=7, A=12, Gmax=3, nvid=1):
        p = ctypes.addressof(arr)
        return lib.fx_vn_match_cost_batch(p, p, nvid, n1, n2, None, None, A, 0.2, 1.0, Gmax, None, None)

    def pred(arr, n1=5, n2=7, A=12, nvid=1):
        p = ctypes.addressof(arr)
        return lib.fx_vn_eval_pred_batch(p, p, nvid, n1, n2, None, None, A, 0.1, None, None, None)
    # nothing to do: no video, or no token / no frame anywhere -> no launch, no error
    assert cost(_video(), nvid=0) == 0 and pred(_video(), nvid=0) == 0
    assert cost(_video(Q=0)) == 0 and pred(_video(T=0, nattn=1)) == 0
    for bad, text in ((dict(nattn=21), b"at most T rows"), (dict(seg_end=0), b"starts and ends"),
                      (dict(G=4), b"Gmax"), (dict(G=0), b"ground-truth"), (dict(lda=13), b"leading dimension"),
                      (dict(ldattn=7), b"leading dimension"), (dict(seg_start=0, seg_end=0), b"one row per frame"),
                      (dict(gl=0), b"bad arguments")):
        assert cost(_video(**bad)) != 0 and text in lib.fx_last_error(), bad
    assert cost(_video(), n1=1500, n2=600) != 0 and b"2048" in lib.fx_last_error()
    assert cost(_video(), A=0) != 0
    for bad, text in ((dict(Q=0), b"bad sizes"), (dict(ldf=11), b"bad sizes"), (dict(pred_off=-1), b"bad sizes"),
                      (dict(seg_id=0), b"one row per frame"), (dict(frame_clogit=0), b"bad arguments")):
        assert pred(_video(**bad)) != 0 and text in lib.fx_last_error(), bad
    assert pred(_video(), n1=1500, n2=600) != 0 and b"2048" in lib.fx_last_error()
    # a good video with NULL tables / outputs is still refused before the launch
    assert cost(_video()) != 0 and pred(_video()) != 0


class _Seq:
    """Stands for an input tensor on a device this machine may not have."""

    def __init__(self, T, cuda=True):
        self.is_cuda, self.shape = cuda, (T, 40)


def _net(match="o2o"):
    vn.set_verb_noun_ids([0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 0, 2], [0, 1, 2, 3, 4, 5, 6, 0, 1, 2, 3, 6])
    cfg = get_cfg_defaults()
    cfg.FACT.update(dict(ntoken=8, block="IU", fpos=True, cmr=0.0, trans=False))
    cfg.Bi.update(dict(hid_dim=48, dropout=0.0, a="sca", a_nhead=4, a_ffdim=48, a_layers=2, a_dim=32,
                       f="m", f_layers=2, f_ln=False, f_dim=24, f_ngp=1))
    cfg.BU.update(dict(f_layers=2, a_nhead=4, s_layers=1))
    cfg.Loss.match = match
    return vn.FACT(cfg, 40, 5, 7)


def test_switch_default_and_guard(monkeypatch):
    assert vn.LOCKSTEP is False
    net = _net()
    assert vn._lockstep_ok(net, [_Seq(50), _Seq(7)]) and vn._lockstep_ok(net, [_Seq(1)])
    assert not vn._lockstep_ok(net, [])
    assert not vn._lockstep_ok(net, [torch.zeros(50, 40)])                     # CPU inputs
    assert not vn._lockstep_ok(net, [_Seq(50), _Seq(7, cuda=False)])
    assert blocks.MAX_LOCKSTEP_VIDEOS == 16
    assert vn._lockstep_ok(net, [_Seq(9)] * 16) and not vn._lockstep_ok(net, [_Seq(9)] * 17)
    net.cfg.FACT.trans = True
    assert not vn._lockstep_ok(net, [_Seq(50)])
    net.cfg.FACT.trans = False
    assert vn._lockstep_ok(net, [_Seq(50)])
    monkeypatch.setattr(vn_vloss, "FUSED_TABLE", False)
    assert not vn._lockstep_ok(net, [_Seq(50)])
    monkeypatch.setattr(vn_vloss, "FUSED_TABLE", True)
    monkeypatch.setattr(vn, "FUSED_LOSS", False)
    assert not vn._lockstep_ok(net, [_Seq(50)])
    monkeypatch.setattr(vn, "FUSED_LOSS", True)
    net.block_list[0].action_branch.layers[0].normalize_before = True          # not a fused-decoder option
    assert not vn._lockstep_ok(net, [_Seq(50)])


def test_cpu_inputs_take_the_per_video_path_with_the_switch_on(monkeypatch):
    monkeypatch.setattr(vn, "LOCKSTEP", True)
    net = _net()

    def boom(*a, **k):
        raise AssertionError("the lockstep pass ran on CPU inputs")
    monkeypatch.setattr(net, "_forward_lockstep", boom)
    seen = []
    monkeypatch.setattr(net, "_forward_one_video", lambda seq, trans=None: seen.append(tuple(seq.shape)) or 1 / 0)
    with pytest.raises(ZeroDivisionError):
        net([torch.zeros(50, 40)], [torch.zeros(50, dtype=torch.long)])
    assert seen == [(50, 1, 40)]
    for blk in net.block_list:
        assert hasattr(blk, "forward_batch")


def test_batch_coefficient_matrix_two_videos_IU():
    Ts, Q, A, sw = [50, 31], 8, 12, 5.0
    S = [[7, 4], [5, 3]]                       # S[block][video]
    rows, coef = vn_vloss.batch_plan(["I", "U"], Ts, S, Q, A, sw)
    per_video = ["frame", "seg", "token", "frame", "seg", "token", "f2a", "a2f"]
    assert [(r[0], r[2]) for r in rows] == [(0, n) for n in per_video] + [(1, n) for n in per_video]
    assert [r[1] for r in rows] == [0, 0, 0, 1, 1, 1, 1, 1] * 2
    nvid, nb, nt = 2, 2, 16
    assert coef.shape == (1 + nvid + nvid * nb, nt) and coef.dtype == np.float32
    np.testing.assert_array_equal(coef[0], np.full(nt, np.float32(1.0 / (nvid * nb))))
    want = np.zeros((1 + nvid + nvid * nb, nt), dtype=np.float32)
    want[0] = 0.25
    want[1, :8] = 0.5                           # video 0: the mean over its two blocks
    want[2, 8:] = 0.5
    want[3, 0:3] = 1.0                          # video 0, block I
    want[4, 3:8] = 1.0                          # video 0, block U
    want[5, 8:11] = 1.0
    want[6, 11:16] = 1.0
    np.testing.assert_array_equal(coef, want)
    # each video's terms carry term_plan's coefficients for its own T and segment counts
    for v in range(nvid):
        one, _ = vn_vloss.term_plan(["I", "U"], Ts[v], [S[0][v], S[1][v]], Q, A, sw)
        assert [r[1:] for r in rows if r[0] == v] == one
    by = {(v, k, name): (c_ce, c_sm) for v, k, name, c_ce, c_sm in rows}
    assert by[(1, 0, "frame")] == (0.25 / 31, sw / (30 * A)) and by[(1, 1, "seg")] == (0.25 / 3, 0.0)
    assert by[(0, 1, "a2f")] == (1.0 / 5, 0.0) and by[(1, 1, "f2a")] == (1.0 / 3, 0.0)
