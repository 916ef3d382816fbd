"""A transcript batch of unequal lengths as ONE lockstep pass (blocks.TRANS_RAGGED, GPU): ragged token rows
through every decoder (fx_decoder_params.tok_off), the X2Y maps, the BiGRU input branch and the loss phase,
against the reference fixtures (tests/golden/make_golden_trans.py, make_golden_trans_ragged.py) and against
the per-video path.  Tolerances are DESIGN.md section 7l's, as tests/test_gpu_trans.py keeps them: loss 2e-5
relative; gradients rtol 2e-3 + 2e-3 x RMS + 1e-6; predictions, matching and segment bounds equal.
"""
import numpy as np
import pytest
import torch

from factmx.models import blocks, vloss
from helpers import load_fixture, tiny_meta
from test_gpu_trans import _Calls, _check_grads, _forbid_per_video_path, _net, _video

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _spy_passes(monkeypatch, net):
    passes = []
    orig = net._forward_batch

    def spy(seq_list, on_a2f=None, transcripts=None):
        passes.append([len(t) for t in transcripts])
        return orig(seq_list, on_a2f, transcripts)
    monkeypatch.setattr(net, "_forward_batch", spy)
    return passes


def test_abc_is_one_pass_vs_reference(monkeypatch):
    """[A, B, C] (5, 5 and 4 transcript entries) with the switch on: ONE _forward_batch call, one term table,
    one prediction launch and one embedding forward, the per-video loss methods forbidden; per-video losses,
    predictions, the segment counts and bounds of every video and the gradients of the batch-mean loss match
    the reference.  (Without the ragged pass: three passes.)"""
    monkeypatch.setattr(blocks, "TRANS_RAGGED", True)
    fx = load_fixture("tiny_trans_batch")
    meta = tiny_meta(fx)
    net = _net(meta)
    _forbid_per_video_path(monkeypatch)
    calls = _Calls(monkeypatch, "fx_loss_terms_fwd", "fx_eval_pred_trans", "fx_token_embed_fwd")
    passes = _spy_passes(monkeypatch, net)
    data = [_video(v) for v in meta["videos"]]
    total, saves = net([d[0] for d in data], [d[1] for d in data], compute_loss=True)
    total.backward()
    torch.cuda.synchronize()
    assert passes == [[5, 5, 4]]
    assert calls.n == dict(fx_loss_terms_fwd=1, fx_eval_pred_trans=1, fx_token_embed_fwd=1)
    np.testing.assert_allclose(total.item(), fx["abc/loss"][0], rtol=2e-5)
    assert len(saves) == 3
    last = net.block_list[-1]
    for v in range(3):
        p = f"abc/vid{v}/"
        np.testing.assert_array_equal(saves[v]["pred"], fx[p + "pred"], err_msg=p)
        np.testing.assert_allclose(saves[v]["loss"]["loss"], fx["abc/video_loss"][v], rtol=2e-5)
        assert net.video_segments[v] == [len(fx[p + "tdu0/seg_start"])]
        tdu = last._vrec[v]["tdu"]
        np.testing.assert_array_equal(tdu.start32.cpu().numpy(), fx[p + "tdu0/seg_start"])
        np.testing.assert_array_equal(tdu.end32.cpu().numpy(), fx[p + "tdu0/seg_end"])
        Q, T = len(fx[p + "transcript"]), meta["videos"][v]["T"]
        assert last._vrec[v]["action_clogit"].shape[0] == Q
        rec = net.block_list[1]._vrec[v]          # (the frame-level update block's views of the packed attention)
        assert rec["a2f_attn"].shape == (1, T, Q) and rec["f2a_attn_logit"].shape == (1, Q, T)
    # the side channels hold the last video's values
    np.testing.assert_array_equal(last.tdu.start32.cpu().numpy(), fx["abc/vid2/tdu0/seg_start"])
    assert last.frame_clogit.shape[0] == meta["videos"][2]["T"] and last.action_clogit.shape[0] == 4
    _check_grads(net, fx, "abc/")


def test_cab_one_pass_vs_per_video_path(monkeypatch):
    """The order [C, A, B] (the short video first) against the per-video path (TRANS_BATCH = False) on the same
    weights: losses to 2e-5 relative, predictions equal."""
    fx = load_fixture("tiny_trans_batch")
    meta = tiny_meta(fx)
    A, B, C = meta["videos"]
    data = [_video(v) for v in (C, A, B)]

    def run(ragged):
        monkeypatch.setattr(blocks, "TRANS_RAGGED", ragged)
        monkeypatch.setattr(blocks, "TRANS_BATCH", ragged)
        net = _net(meta)
        passes = _spy_passes(monkeypatch, net)
        total, saves = net([d[0] for d in data], [d[1] for d in data], compute_loss=True)
        total.backward()
        torch.cuda.synchronize()
        return total.item(), [dict(s) for s in saves], passes
    l1, s1, p1 = run(True)
    l0, s0, p0 = run(False)
    assert p1 == [[4, 5, 5]] and p0 == []
    np.testing.assert_allclose(l1, l0, rtol=2e-5)
    for v in range(3):
        np.testing.assert_array_equal(s1[v]["pred"], s0[v]["pred"])
        np.testing.assert_allclose(s1[v]["loss"]["loss"], s0[v]["loss"]["loss"], rtol=2e-5)


def test_prediction_only_and_eval_mode(monkeypatch):
    monkeypatch.setattr(blocks, "TRANS_RAGGED", True)
    fx = load_fixture("tiny_trans_batch")
    meta = tiny_meta(fx)
    net = _net(meta)
    passes = _spy_passes(monkeypatch, net)
    data = [_video(v) for v in meta["videos"]]
    seqs, labels = [d[0] for d in data], [d[1] for d in data]
    saves = net(seqs, labels, compute_loss=False)
    net.eval()
    with torch.no_grad():
        saves_e = net(seqs, labels, compute_loss=False)
    assert passes == [[5, 5, 4], [5, 5, 4]]
    for v in range(3):
        np.testing.assert_array_equal(saves[v]["pred"], fx[f"abc/vid{v}/pred"])
        np.testing.assert_array_equal(saves_e[v]["pred"], fx[f"abc/vid{v}/pred"])


def test_a_table_that_does_not_fit_falls_back_per_video(monkeypatch):
    """The TableTooLarge way out of a ragged pass (the limit lowered to 3 matched columns): the lockstep forward
    is kept, losses and predictions run per video on its outputs, results in the same bounds."""
    from factmx import native as nx
    monkeypatch.setattr(blocks, "TRANS_RAGGED", True)
    monkeypatch.setattr(nx, "LOSS_MAXK", 3)
    fx = load_fixture("tiny_trans_batch")
    meta = tiny_meta(fx)
    net = _net(meta)
    calls = _Calls(monkeypatch, "fx_loss_terms_fwd", "fx_token_embed_fwd")
    data = [_video(v) for v in meta["videos"]]
    total, saves = net([d[0] for d in data], [d[1] for d in data], compute_loss=True)
    total.backward()
    torch.cuda.synchronize()
    assert calls.n == dict(fx_loss_terms_fwd=0, fx_token_embed_fwd=1)
    np.testing.assert_allclose(total.item(), fx["abc/loss"][0], rtol=2e-5)
    for v in range(3):
        np.testing.assert_array_equal(saves[v]["pred"], fx[f"abc/vid{v}/pred"])
        np.testing.assert_allclose(saves[v]["loss"]["loss"], fx["abc/video_loss"][v], rtol=2e-5)
    _check_grads(net, fx, "abc/")


def test_gru_branch_and_matching_cost_block_vs_reference(monkeypatch):
    """Block iU, gru_om, o2o on [A, C] (5 and 4 entries): the BiGRU input branch over ragged token sequences
    and the (videos, longest transcript, most segments) matching cost block in ONE fx_match_cost launch.  The
    matching equals the reference's, the rest is within the bounds."""
    monkeypatch.setattr(blocks, "TRANS_RAGGED", True)
    fx = load_fixture("tiny_trans_ragged")
    meta = tiny_meta(fx)
    net = _net(meta)
    assert isinstance(net.block_list[0].action_branch, blocks.basic.ActionUpdate_GRU)
    _forbid_per_video_path(monkeypatch)
    calls = _Calls(monkeypatch, "fx_loss_terms_fwd", "fx_eval_pred_trans", "fx_match_cost")
    passes = _spy_passes(monkeypatch, net)
    got = {}
    orig = vloss.EarlyMatch.matches

    def spy(self, Q=None):
        got["m"] = orig(self, Q)
        return got["m"]
    monkeypatch.setattr(vloss.EarlyMatch, "matches", spy)
    data = [_video(v) for v in meta["videos"]]
    total, saves = net([d[0] for d in data], [d[1] for d in data], compute_loss=True)
    total.backward()
    torch.cuda.synchronize()
    assert passes == [[5, 4]]
    assert calls.n == dict(fx_loss_terms_fwd=1, fx_eval_pred_trans=1, fx_match_cost=1)
    np.testing.assert_allclose(total.item(), fx["ac/loss"][0], rtol=2e-5)
    last = net.block_list[-1]
    for v in range(2):
        p = f"ac/vid{v}/"
        np.testing.assert_array_equal(got["m"][v][0], fx[p + "match_a"])
        np.testing.assert_array_equal(got["m"][v][1], fx[p + "match_s"])
        np.testing.assert_array_equal(saves[v]["pred"], fx[p + "pred"], err_msg=p)
        np.testing.assert_allclose(saves[v]["loss"]["loss"], fx["ac/video_loss"][v], rtol=2e-5)
        assert net.video_segments[v] == [len(fx[p + "tdu0/seg_start"])]
        tdu = last._vrec[v]["tdu"]
        np.testing.assert_array_equal(tdu.start32.cpu().numpy(), fx[p + "tdu0/seg_start"])
        np.testing.assert_array_equal(tdu.end32.cpu().numpy(), fx[p + "tdu0/seg_end"])
    _check_grads(net, fx, "ac/")
