"""Transcript-conditioned FACT (``FACT.trans``) on the lockstep pass and the fused loss phase (GPU), against
the fixtures captured from the reference (tests/golden/make_golden_trans.py).

Tolerances are DESIGN.md section 7l's, kept as they are: loss 2e-5 relative; gradients rtol 2e-3 + 2e-3 x RMS
+ 1e-6; logits 1e-4 + 1e-4 |ref|, attention 1e-5; predictions, matching and segment bounds equal.  The
reference's own float32 run sits 1.5e-7 (loss), 4e-6 (logits), 1.8e-7 (attention) from its float64 run and its
gradients use 3.5 % of their bound (make_golden_trans.py --spread): all under one third
of the bounds, which therefore stand.  The fixtures' margin conditions (segmentation >= 1e-3 relative;
prediction >= 100 x the float32 difference of the blended probability) make the integer outputs exact.
"""
import numpy as np
import pytest
import torch

import paramgen as pg
from factmx import native as nx
from factmx.models import blocks, vloss
from factmx.models import loss as loss_mod
from factmx.models.loss import MatchCriterion
from helpers import load_fixture, tiny_meta, cfg_from_meta, check_grad

pytestmark = pytest.mark.gpu
DEV = "cuda"
TERM_METHODS = ("action_token_loss", "cross_attn_loss", "cross_attn_loss_tdu", "frame_terms", "seg_terms",
                "attn_terms", "frame_loss", "frame_loss_tdu", "match")


def _video(v, D=40):
    feats, label = pg.segmented_video(v["T"], D, v["classes"], v["nseg"], seed=v["seed"], noise=v["noise"])
    return torch.from_numpy(feats).float().to(DEV), torch.from_numpy(label).to(DEV)


def _net(meta, cfg=None, clip=False, text=None):
    cfg = cfg_from_meta(meta) if cfg is None else cfg
    net = blocks.FACT_CLIP(cfg, meta["D"], meta["C"], text_embeddings=text) if clip else \
        blocks.FACT(cfg, meta["D"], meta["C"])
    with torch.no_grad():
        for n, p in net.named_parameters():
            p.copy_(torch.from_numpy(pg.param_value(n, p.shape, meta["seed"])))
    net.mcriterion = MatchCriterion(cfg, meta["C"], [])
    return net.to(DEV).train()


class _Calls:
    """Counts the calls of library entry points (the bound functions of the loaded library, patched in place)."""

    def __init__(self, monkeypatch, *names):
        lib = nx.load()
        self.n = {k: 0 for k in names}
        for k in names:
            monkeypatch.setattr(lib, k, self._wrap(k, getattr(lib, k)))

    def _wrap(self, k, fn):
        def call(*a):
            self.n[k] += 1
            return fn(*a)
        return call


def _forbid_per_video_path(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the per-video loss / prediction path ran")
    for name in TERM_METHODS:
        monkeypatch.setattr(loss_mod.MatchCriterion, name, boom)
    monkeypatch.setattr(blocks.Block, "_eval_w_transcript", staticmethod(boom))


def _check_grads(net, fx, prefix=""):
    for n, prm in net.named_parameters():
        g = prm.grad
        assert g is not None, n
        rms = float(fx[f"{prefix}gradsum/{n}"][1]) / np.sqrt(g.numel())
        check_grad(fx, prefix, n, g.cpu(), rtol=2e-3, atol=2e-3 * rms + 1e-6)


def _check_side(net, fx):
    for i, blk in enumerate(net.block_list):
        p = f"block{i}/"
        for k in ("frame_clogit", "action_clogit", "seg_clogit"):
            if p + k in fx:
                np.testing.assert_allclose(getattr(blk, k)[:, 0].detach().cpu().numpy(), fx[p + k], rtol=1e-4, atol=1e-4,
                                           err_msg=p + k)
        if p + "seg_start" in fx:
            np.testing.assert_array_equal(blk.tdu.start32.cpu().numpy(), fx[p + "seg_start"], err_msg=p)
            np.testing.assert_array_equal(blk.tdu.end32.cpu().numpy(), fx[p + "seg_end"], err_msg=p)
        if p + "a2f_attn" in fx:
            np.testing.assert_allclose(blk.a2f_attn[0].detach().cpu().numpy(), fx[p + "a2f_attn"], atol=1e-5)
            for k in ("f2a_attn_logit", "a2f_attn_logit"):
                np.testing.assert_allclose(getattr(blk, k)[0].detach().cpu().numpy(), fx[p + k], rtol=1e-4, atol=1e-4,
                                           err_msg=p + k)


def test_tiny_trans_vs_reference_on_the_fused_path(monkeypatch):
    """Loss, predictions, segment bounds, side tensors and every gradient (``action_embed.weight`` included)
    of video A against the reference, with the per-video loss methods and the eager transcript prediction
    forbidden: one fx_loss_terms_fwd, one fx_eval_pred_trans, one embedding forward.  (Fails without the
    lockstep transcript path: transcript models then run the per-video methods.)"""
    fx = load_fixture("tiny_trans")
    meta = tiny_meta(fx)
    net = _net(meta)
    assert {n: list(p.shape) for n, p in net.named_parameters()} == meta["param_shapes"]
    _forbid_per_video_path(monkeypatch)
    calls = _Calls(monkeypatch, "fx_loss_terms_fwd", "fx_eval_pred_trans", "fx_token_embed_fwd", "fx_eval_pred",
                   "fx_match_cost")
    seq, label = _video(meta["video"])
    total, saves = net([seq], [label], compute_loss=True)
    total.backward()
    torch.cuda.synchronize()
    assert calls.n == dict(fx_loss_terms_fwd=1, fx_eval_pred_trans=1, fx_token_embed_fwd=1, fx_eval_pred=0,
                           fx_match_cost=0)                       # (seq matching needs no cost launch)
    np.testing.assert_array_equal(saves[0]["pred"], fx["pred"])
    np.testing.assert_allclose(total.item(), fx["loss"][0], rtol=2e-5)
    np.testing.assert_allclose(saves[0]["loss"]["loss"], fx["loss"][0], rtol=2e-5)
    assert net.video_segments == [[len(fx["block2/seg_start"])]]
    _check_side(net, fx)
    _check_grads(net, fx)
    assert "grad/action_embed.weight" in fx and net.action_embed.weight.grad.abs().sum() > 0


@pytest.mark.parametrize("tag,npass", [("ab", 1), ("abc", 3)])
def test_batches_vs_reference(monkeypatch, tag, npass):
    """[A, B] (equal transcript lengths) is ONE _forward_batch call and one term table; [A, B, C] (C has four
    entries) is three passes of one video.  Per-video losses, predictions, segments and the gradients of the
    batch-mean loss match the reference either way."""
    fx = load_fixture("tiny_trans_batch")
    meta = tiny_meta(fx)
    net = _net(meta)
    _forbid_per_video_path(monkeypatch)
    calls = _Calls(monkeypatch, "fx_loss_terms_fwd", "fx_eval_pred_trans", "fx_token_embed_fwd")
    passes = []
    orig = net._forward_batch

    def spy(seq_list, on_a2f=None, transcripts=None):
        passes.append([len(t) for t in transcripts])
        return orig(seq_list, on_a2f, transcripts)
    monkeypatch.setattr(net, "_forward_batch", spy)
    vids = meta["videos"][:len(tag)]
    data = [_video(v) for v in vids]
    total, saves = net([d[0] for d in data], [d[1] for d in data], compute_loss=True)
    total.backward()
    torch.cuda.synchronize()
    assert passes == ([[5, 5]] if tag == "ab" else [[5], [5], [4]])
    assert calls.n == dict(fx_loss_terms_fwd=npass, fx_eval_pred_trans=npass, fx_token_embed_fwd=npass)
    np.testing.assert_allclose(total.item(), fx[f"{tag}/loss"][0], rtol=2e-5)
    assert len(saves) == len(vids)
    for v in range(len(vids)):
        p = f"{tag}/vid{v}/"
        np.testing.assert_array_equal(saves[v]["pred"], fx[p + "pred"], err_msg=p)
        np.testing.assert_allclose(saves[v]["loss"]["loss"], fx[f"{tag}/video_loss"][v], rtol=2e-5)
        assert net.video_segments[v] == [len(fx[p + "tdu0/seg_start"])]
    last = net.block_list[-1]
    if tag == "ab":          # every video's segment bounds of the one pass
        for v in range(2):
            tdu = last._vrec[v]["tdu"]
            np.testing.assert_array_equal(tdu.start32.cpu().numpy(), fx[f"ab/vid{v}/tdu0/seg_start"])
            np.testing.assert_array_equal(tdu.end32.cpu().numpy(), fx[f"ab/vid{v}/tdu0/seg_end"])
    # the side channels hold the last video's values
    v = len(vids) - 1
    np.testing.assert_array_equal(last.tdu.start32.cpu().numpy(), fx[f"{tag}/vid{v}/tdu0/seg_start"])
    assert last.frame_clogit.shape[0] == vids[v]["T"]
    _check_grads(net, fx, tag + "/")


def test_tiny_trans_gru_vs_reference(monkeypatch):
    """Block iU with the GRU input branch (gru_om) and Hungarian matching: the matching equal, the rest in bounds."""
    fx = load_fixture("tiny_trans_gru")
    meta = tiny_meta(fx)
    net = _net(meta)
    assert isinstance(net.block_list[0].action_branch, blocks.basic.ActionUpdate_GRU)
    _forbid_per_video_path(monkeypatch)
    calls = _Calls(monkeypatch, "fx_loss_terms_fwd", "fx_eval_pred_trans", "fx_match_cost")
    got = {}
    orig = vloss.EarlyMatch.matches

    def spy(self, Q):
        got["m"] = orig(self, Q)
        return got["m"]
    monkeypatch.setattr(vloss.EarlyMatch, "matches", spy)
    seq, label = _video(meta["video"])
    total, saves = net([seq], [label], compute_loss=True)
    total.backward()
    torch.cuda.synchronize()
    assert calls.n == dict(fx_loss_terms_fwd=1, fx_eval_pred_trans=1, fx_match_cost=1)
    np.testing.assert_array_equal(got["m"][0][0], fx["match_a"])
    np.testing.assert_array_equal(got["m"][0][1], fx["match_s"])
    np.testing.assert_array_equal(saves[0]["pred"], fx["pred"])
    np.testing.assert_allclose(total.item(), fx["loss"][0], rtol=2e-5)
    _check_side(net, fx)
    _check_grads(net, fx)


def test_per_video_path_stays_in_the_same_bounds(monkeypatch):
    """blocks.TRANS_BATCH = False restores the per-video path; it meets the fixture in the same bounds."""
    monkeypatch.setattr(blocks, "TRANS_BATCH", False)
    fx = load_fixture("tiny_trans")
    meta = tiny_meta(fx)
    net = _net(meta)
    calls = _Calls(monkeypatch, "fx_loss_terms_fwd", "fx_eval_pred_trans", "fx_token_embed_fwd")
    seq, label = _video(meta["video"])
    total, saves = net([seq], [label], compute_loss=True)
    total.backward()
    torch.cuda.synchronize()
    assert calls.n == dict(fx_loss_terms_fwd=0, fx_eval_pred_trans=0, fx_token_embed_fwd=0)
    np.testing.assert_array_equal(saves[0]["pred"], fx["pred"])
    np.testing.assert_allclose(total.item(), fx["loss"][0], rtol=2e-5)
    _check_side(net, fx)
    _check_grads(net, fx)


def test_fact_clip_with_text_new_path_vs_per_video_path(monkeypatch):
    """FACT_CLIP + FACT.trans + text embeddings: the lockstep path against the per-video path
    (TRANS_BATCH = False) on the same weights -- predictions equal, loss within 2e-5 relative, gradients within
    rtol 2e-3 + 2e-3 x RMS + 1e-6.  There is NO reference fixture for this case: the comparison is between the
    project's two paths (the reference's eval_with_clip ignores the transcript, so fx_eval_pred is used)."""
    fx = load_fixture("tiny_trans")
    meta = tiny_meta(fx)
    text = torch.from_numpy(pg.text_embeddings(meta["C"], seed=meta["seed"])).float()
    seq, label = _video(meta["video"])

    def run(batch):
        monkeypatch.setattr(blocks, "TRANS_BATCH", batch)
        cfg = cfg_from_meta(meta)
        cfg.CLIP.projection_dropout = 0.0
        net = _net(meta, cfg, clip=True, text=text)
        total, saves = net([seq], [label], compute_loss=True)
        total.backward()
        torch.cuda.synchronize()
        return total.item(), dict(saves[0]), {n: p.grad.double().cpu() for n, p in net.named_parameters()}
    calls = _Calls(monkeypatch, "fx_eval_pred", "fx_eval_pred_trans", "fx_loss_terms_fwd")
    l1, s1, g1 = run(True)
    assert calls.n == dict(fx_eval_pred=1, fx_eval_pred_trans=0, fx_loss_terms_fwd=1)
    l0, s0, g0 = run(False)
    np.testing.assert_array_equal(s1["pred"], s0["pred"])
    np.testing.assert_allclose(l1, l0, rtol=2e-5)
    for k in ("loss", "fact_loss", "contrastive_loss"):
        np.testing.assert_allclose(s1["loss"][k], s0["loss"][k], rtol=2e-5, err_msg=k)
    for n, r in g0.items():
        rms = float(np.sqrt((r * r).mean()))
        np.testing.assert_allclose(g1[n].numpy(), r.numpy(), rtol=2e-3, atol=2e-3 * rms + 1e-6, err_msg=n)


def test_prediction_only_and_eval_mode_agree():
    fx = load_fixture("tiny_trans")
    meta = tiny_meta(fx)
    net = _net(meta)
    seq, label = _video(meta["video"])
    saves = net([seq], [label], compute_loss=False)
    np.testing.assert_array_equal(saves[0]["pred"], fx["pred"])
    net.eval()
    with torch.no_grad():
        saves = net([seq], [label], compute_loss=False)
    np.testing.assert_array_equal(saves[0]["pred"], fx["pred"])
    ev = net.block_list[-1].eval(torch.from_numpy(fx["transcript"]).to(DEV))      # the module's own eager eval
    np.testing.assert_array_equal(ev.cpu().numpy(), fx["pred"])


def test_training_step_with_masking_and_dropout_is_finite():
    fx = load_fixture("tiny_trans_batch")
    meta = tiny_meta(fx)
    cfg = cfg_from_meta(meta)
    cfg.FACT.cmr = 0.5
    cfg.Bi.dropout = 0.2
    cfg.TM.update(dict(use=True, t=30, m=2, p=0.1))
    net = _net(meta, cfg)
    data = [_video(v) for v in meta["videos"][:2]]
    torch.manual_seed(7)
    total, saves = net([d[0] for d in data], [d[1] for d in data], compute_loss=True)
    total.backward()
    torch.cuda.synchronize()
    assert np.isfinite(total.item())
    for s, d in zip(saves, data):
        assert set(s["pred"].tolist()) <= set(d[1].tolist())
    for n, p in net.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n


def test_inference_without_a_criterion_runs_per_video(monkeypatch):
    """A freshly constructed model (``mcriterion`` None, as the constructor leaves it) predicting with
    compute_loss=False: the fused loss phase does not cover it, so it runs video by video as before."""
    fx = load_fixture("tiny_trans")
    meta = tiny_meta(fx)
    net = _net(meta)
    net.mcriterion = None
    calls = _Calls(monkeypatch, "fx_eval_pred_trans", "fx_token_embed_fwd")
    seq, label = _video(meta["video"])
    for mode in (net.train, net.eval):
        mode()
        with torch.no_grad():
            saves = net([seq], [label], compute_loss=False)
        np.testing.assert_array_equal(saves[0]["pred"], fx["pred"])
    assert calls.n == dict(fx_eval_pred_trans=0, fx_token_embed_fwd=0)


def test_fused_loss_switch_off_runs_per_video(monkeypatch):
    """blocks.FUSED_LOSS = False (the A/B switch of the loss phase) keeps working for transcript models: the
    per-video path, inside the same bounds."""
    monkeypatch.setattr(blocks, "FUSED_LOSS", False)
    fx = load_fixture("tiny_trans")
    meta = tiny_meta(fx)
    net = _net(meta)
    calls = _Calls(monkeypatch, "fx_loss_terms_fwd", "fx_eval_pred_trans", "fx_token_embed_fwd")
    seq, label = _video(meta["video"])
    total, saves = net([seq], [label], compute_loss=True)
    total.backward()
    torch.cuda.synchronize()
    assert calls.n == dict(fx_loss_terms_fwd=0, fx_eval_pred_trans=0, fx_token_embed_fwd=0)
    np.testing.assert_array_equal(saves[0]["pred"], fx["pred"])
    np.testing.assert_allclose(total.item(), fx["loss"][0], rtol=2e-5)
    _check_grads(net, fx)


def test_a_table_that_does_not_fit_falls_back_per_video(monkeypatch):
    """More matched columns than the term table holds (here the limit is lowered to 3 for the 5 transcript
    entries): the pass keeps its lockstep forward, and its losses and predictions run per video on those
    outputs, as the learned-query path does -- no error, results in the same bounds."""
    monkeypatch.setattr(nx, "LOSS_MAXK", 3)
    fx = load_fixture("tiny_trans_batch")
    meta = tiny_meta(fx)
    net = _net(meta)
    calls = _Calls(monkeypatch, "fx_loss_terms_fwd", "fx_token_embed_fwd")
    data = [_video(v) for v in meta["videos"][:2]]
    total, saves = net([d[0] for d in data], [d[1] for d in data], compute_loss=True)
    total.backward()
    torch.cuda.synchronize()
    assert calls.n == dict(fx_loss_terms_fwd=0, fx_token_embed_fwd=1)
    np.testing.assert_allclose(total.item(), fx["ab/loss"][0], rtol=2e-5)
    for v in range(2):
        np.testing.assert_array_equal(saves[v]["pred"], fx[f"ab/vid{v}/pred"])
        np.testing.assert_allclose(saves[v]["loss"]["loss"], fx["ab/video_loss"][v], rtol=2e-5)
        assert net.video_segments[v] == [len(fx[f"ab/vid{v}/tdu0/seg_start"])]
    _check_grads(net, fx, "ab/")
