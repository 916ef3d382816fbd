"""The verb/noun loss surface of models/loss.py on CPU tensors (no kernels): the ``vn_*_terms`` of
``MatchCriterion`` are the reference's ``is_logit=False`` terms on the materialised action
log-probabilities, and the (T, A) one-hot of the frame labels is built only when it is read."""
import numpy as np
import pytest
import torch

from factmx.configs import get_cfg_defaults
from factmx.functional import VerbNounMap
from factmx.models import loss as L
from factmx.models.basic import TemporalDownsampleUpsample
from factmx.models.loss import MatchCriterion

V, N = 5, 7
VIDS = [0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 0, 2]
NIDS = [0, 1, 2, 3, 4, 5, 6, 0, 1, 2, 3, 6]
A = len(VIDS)
LABEL = [3, 3, 3, 7, 7, 0, 0, 0, 0, 11, 11, 3, 3, 5, 5, 5, 5]
SEG_START = [0, 2, 5, 6, 9, 13]          # the TDU's own segmentation: not the label's
SEG_END = [1, 4, 5, 8, 12, 16]


def _materialised(cl, n1, action):
    """blocks_SepVerbNoun.py:189-224 in fp64."""
    lv, ln = torch.log_softmax(cl[:, :n1], -1), torch.log_softmax(cl[:, n1:], -1)
    lp = lv[:, VIDS] + ln[:, NIDS]
    if action:
        lp = torch.cat([lp, (lv[:, -1] + ln[:, -1]).unsqueeze(-1)], -1)
    return lp


@pytest.fixture()
def crit():
    cfg = get_cfg_defaults()
    cfg.Loss.nullw = 0.3
    cfg.Loss.bgw = 0.5
    c = MatchCriterion(cfg, A, bg_ids=[0])
    c.set_label(torch.tensor(LABEL))
    return c


def _r(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 2.0


def _tdu():
    T = len(LABEL)
    sid = torch.zeros(T, dtype=torch.int32)
    for s, (a, b) in enumerate(zip(SEG_START, SEG_END)):
        sid[a:b + 1] = s
    return TemporalDownsampleUpsample(sid, torch.tensor(SEG_START, dtype=torch.int32),
                                      torch.tensor(SEG_END, dtype=torch.int32))


def test_onehot_class_label_is_lazy(crit):
    assert crit.__dict__["_onehot_class_label"] is None          # set_label did not build it
    oh = crit.onehot_class_label
    assert torch.equal(oh, L._onehot(torch.tensor(LABEL), A))
    assert oh.dtype == torch.float32 and tuple(oh.shape) == (len(LABEL), A)
    assert crit.onehot_class_label is oh                          # built once
    crit.set_label(torch.tensor(LABEL[:5]))
    assert crit.__dict__["_onehot_class_label"] is None
    assert tuple(crit.onehot_class_label.shape) == (5, A)


@pytest.mark.parametrize("sw", [0.0, 5.0])
def test_vn_frame_terms_cpu(crit, sw):
    m = VerbNounMap(VIDS, NIDS)
    cl = _r(len(LABEL), V + N, seed=1)
    lp = _materialised(cl, V, False)
    want = 0.25 * crit.frame_loss(lp, is_logit=False) + sw * L.smooth_loss(lp.unsqueeze(0), is_logit=False)
    got = crit.vn_frame_terms(cl.unsqueeze(1), m, ce_coef=0.25, sm_coef=sw)
    np.testing.assert_allclose(float(got), float(want), rtol=1e-12)
    assert crit.__dict__["_onehot_class_label"] is not None       # the eager CPU form reads it


def test_vn_seg_terms_cpu(crit):
    m = VerbNounMap(VIDS, NIDS)
    tdu = _tdu()
    cl = _r(tdu.num_seg, V + N, seed=2)
    lp = _materialised(cl, V, False)
    want = 0.5 * crit.frame_loss_tdu(lp.unsqueeze(1), tdu, is_logit=False)
    got = crit.vn_seg_terms(cl.unsqueeze(1), m, tdu, ce_coef=0.5)
    np.testing.assert_allclose(float(got), float(want), rtol=1e-12)


def test_vn_token_terms_cpu(crit):
    from factmx.models.blocks_SepVerbNoun import Block
    m = VerbNounMap(VIDS, NIDS)
    Q = 9
    cl = _r(Q, V + N + 2, seed=3)
    lp = _materialised(cl, V + 1, True)
    S = int(crit.transcript.shape[0])
    match = (torch.tensor([4, 0, 7, 2, 8, 5][:S]), torch.arange(S)[:6])
    want = Block.action_token_loss(None, crit, match, lp.unsqueeze(1))
    got = crit.vn_token_terms(match, cl.unsqueeze(1), m, 1.0)
    np.testing.assert_allclose(float(got), float(want), rtol=1e-12)
    np.testing.assert_allclose(float(crit.vn_token_terms(match, cl, m, 0.5)), 0.5 * float(want), rtol=1e-12)


def test_vn_terms_refuse_heads_that_do_not_fit(crit):
    m = VerbNounMap(VIDS, NIDS)
    with pytest.raises(ValueError):
        crit.vn_frame_terms(_r(len(LABEL), V + N + 1), m)
