"""The verb/noun model's one-table loss phase: what is declared, and its host-side logic (CPU)."""
import os

import numpy as np
import torch

from factmx import native as nx
from factmx.configs import get_cfg_defaults
from factmx.models import blocks_SepVerbNoun as vn
from factmx.models import vn_vloss
from factmx.models.basic import TemporalDownsampleUpsample
from factmx.models.loss import MatchCriterion
from factmx.models.vloss import gt_segments, class_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_binding_declare_the_new_surface():
    with open(os.path.join(ROOT, "include", "factmx.h")) as fp:
        header = fp.read()
    assert "int fx_vn_match_cost(" in header
    assert "FX_TERM_VNCLASS = 3" in header and "typedef struct fx_vn_term" in header
    assert "const fx_vn_term* vn;" in header.split("typedef struct fx_loss_term")[1]
    assert "fx_vn_match_cost" in nx.SIGNATURES
    assert nx.TERM_VNCLASS == 3 and nx.VnTerm in nx.ABI_STRUCTS
    names = [f[0] for f in nx.LossTerm._fields_]
    assert names[-2:] == ["vn", "vn_host"]
    assert vn_vloss.FUSED_TABLE in (True, False)


def _tdu(lens):
    lens = torch.tensor(lens)
    en = torch.cumsum(lens, 0) - 1
    st = en - lens + 1
    sid = torch.repeat_interleave(torch.arange(len(lens)), lens)
    return TemporalDownsampleUpsample(sid.to(torch.int32), st.to(torch.int32), en.to(torch.int32))


def _criterion(kind, label):
    cfg = get_cfg_defaults()
    cfg.Loss.match = kind
    cfg.Loss.pc, cfg.Loss.a2fc = 0.2, 1.0
    crit = MatchCriterion(cfg, 6, [])
    crit.set_label(label)
    return crit


def test_segment_level_match_equals_the_frame_level_match_on_cpu():
    label = torch.from_numpy(np.repeat([3, 1, 3, 0, 5, 1], [9, 4, 11, 6, 2, 8]))
    T, Q = len(label), 8
    tdu = _tdu([5, 1, 7, 12, 3, T - 28])
    g = torch.Generator().manual_seed(0)
    seg_attn = torch.softmax(torch.randn(1, tdu.num_seg, Q, generator=g) * 2, -1)
    p = torch.softmax(torch.randn(Q, 1, 7, generator=g) * 2, -1)
    for kind in ("o2o", "o2m"):
        want = _criterion(kind, label).match(p, tdu.attn_seg2frame(seg_attn))
        got = _criterion(kind, label).match(p, seg_attn, tdu=tdu)
        vnm = vn.fxf.VerbNounMap([0, 1, 2, 0, 1, 2], [0, 0, 0, 1, 1, 1])
        got_vn = _criterion(kind, label).match(p, seg_attn, tdu=tdu, vn=(torch.zeros(Q, 1, 7), vnm))
        for pair in (got, got_vn):
            assert pair[0].dtype == torch.int64 and pair[1].dtype == torch.int64
            assert torch.equal(pair[0], want[0]) and torch.equal(pair[1], want[1])
        assert len(want[1]) == 6


def test_ground_truth_intervals_on_the_device_form():
    label = torch.from_numpy(np.repeat([3, 1, 3, 0], [9, 1, 11, 6]))
    crit = _criterion("o2o", label)
    gs, ge, gl = crit.gt_device()
    hs, he, hl = gt_segments(label.numpy())
    assert gs.dtype == torch.int32
    np.testing.assert_array_equal(gs.numpy(), hs)
    np.testing.assert_array_equal(ge.numpy(), he)
    np.testing.assert_array_equal(gl.numpy(), hl)


def test_table_plan_coefficients():
    T, Q, A, sw = 50, 8, 12, 5.0
    rows, coef = vn_vloss.term_plan(["I", "U", "U"], T, [7, 5, 4], Q, A, sw)
    assert [r[1] for r in rows] == ["frame", "seg", "token"] + ["frame", "seg", "token", "f2a", "a2f"] * 2
    assert coef.shape == (4, 13)
    by = {(k, name): (c_ce, c_sm) for k, name, c_ce, c_sm in rows}
    assert by[(0, "frame")] == (0.25 / T, sw / ((T - 1) * A))
    assert by[(1, "seg")] == (0.25 / 5, 0.0) and by[(2, "seg")] == (0.25 / 4, 0.0)
    assert by[(1, "token")] == (0.5 / Q, 0.0)
    assert by[(1, "f2a")] == (1.0 / 5, 0.0) and by[(2, "a2f")] == (1.0 / 4, 0.0)
    np.testing.assert_allclose(coef[0], np.full(13, 1.0 / 3, dtype=np.float32))
    for i, (k, _, _, _) in enumerate(rows):
        np.testing.assert_array_equal(coef[1:, i], np.eye(3)[k])
    # no smooth term without a weight or with a single frame
    assert vn_vloss.term_plan(["I"], 1, [1], Q, A, sw)[0][0][3] == 0.0
    assert vn_vloss.term_plan(["I"], T, [1], Q, A, 0.0)[0][0][3] == 0.0


def test_match_tables_targets_and_k_limit():
    label = np.repeat([3, 1, 3, 0], [9, 1, 11, 6])
    crit = _criterion("o2m", torch.from_numpy(label))
    gts = gt_segments(label)
    A, Q = 6, 5
    cw = class_weights(crit, A + 1)
    match = (torch.tensor([4, 0, 4, 2]), torch.tensor([0, 1, 2, 3]))     # token 4 takes both segments of action 3
    mt = vn_vloss.match_tables(crit, gts, match, Q, A, cw)
    assert mt["K"] == 4
    np.testing.assert_array_equal(mt["tgt"], [1, A, 0, A, 3])
    np.testing.assert_array_equal(mt["ka"], [4, 0, 4, 2])
    np.testing.assert_array_equal(mt["kgs"], [0, 9, 10, 21])
    np.testing.assert_array_equal(mt["kge"], [8, 9, 20, 26])
    np.testing.assert_array_equal(mt["ksw"], np.ones(4, dtype=np.float32))
    assert mt["tgt"].dtype == np.int32 and mt["ka"].dtype == np.int32
    # more matched columns than an attention term holds: no table, the caller takes the per-term path
    K = nx.LOSS_MAXK + 1
    big = np.repeat(np.arange(K) % A, 2)
    big[1::2] = (big[1::2] + 1) % A
    crit = _criterion("o2m", torch.from_numpy(big))
    gts = gt_segments(big)
    assert len(gts[0]) > nx.LOSS_MAXK
    n = len(gts[0])
    assert vn_vloss.match_tables(crit, gts, (torch.zeros(n, dtype=torch.int64), torch.arange(n)), Q, A, cw) is None


def test_attention_side_channels_are_lazy():
    assert vn_vloss.FUSED_TABLE in (True, False)
    blk = vn.Block()
    tdu = _tdu([2, 1, 4])
    g = torch.Generator().manual_seed(1)
    a2f = torch.softmax(torch.randn(1, 3, 5, generator=g), -1)
    f2a = torch.softmax(torch.randn(1, 3, 5, generator=g), 1)
    blk._save_attn(tdu, f2a, a2f)
    assert blk.a2f_seg_attn is a2f and blk.f2a_seg_attn is f2a
    assert not torch.is_tensor(blk.__dict__["_lz_a2f_attn"]) and not torch.is_tensor(blk.__dict__["_lz_f2a_attn"])
    got = blk.a2f_attn
    assert torch.equal(got, tdu.attn_seg2frame(a2f)) and tuple(got.shape) == (1, 7, 5)
    assert blk.a2f_attn is got and torch.is_tensor(blk.__dict__["_lz_a2f_attn"])
    assert torch.equal(blk.f2a_attn, tdu.attn_seg2frame(f2a).transpose(2, 1)) and tuple(blk.f2a_attn.shape) == (1, 5, 7)
    blk._save_attn(None, None, None)
    assert blk.a2f_attn is None and blk.f2a_attn is None
