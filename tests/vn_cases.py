"""Shared builders of the verb/noun matching-cost and term-table tests (no test in here): inputs on
the host and the float64 restatement of the reference lines on the materialised tensors, the
frames x tokens x segments cube of a2f_soft_iou (loss.py:91-106) included.  ``dtype`` / ``device`` let
the same restatement run in float32 on the CPU (DESIGN.md section 7n records its distance from float64).
"""
import numpy as np
import torch
from scipy.optimize import linear_sum_assignment

from factmx.models.loss import one_to_many_match

BOUND = 2e-5          # entries and gradients: BOUND * (1 + max|ref|); scalars: rtol BOUND


def mapping(V, N, A, seed=0):
    """A verb / noun ids that reach the last verb and the last noun; with few pairs some repeat."""
    rng = np.random.default_rng(seed)
    vids, nids = rng.integers(0, V, A), rng.integers(0, N, A)
    vids[-1], nids[-1] = V - 1, N - 1
    return vids.tolist(), nids.tolist()


def ref_logp(cl, vids, nids, n1, action):
    lv, ln = torch.log_softmax(cl[:, :n1], -1), torch.log_softmax(cl[:, n1:], -1)
    a = lv[:, vids] + ln[:, nids]
    if action:
        a = torch.cat([a, (lv[:, -1] + ln[:, -1]).unsqueeze(-1)], -1)
    return a


def cuts(total, parts, rng):
    """``parts`` positive lengths summing to ``total``."""
    assert 1 <= parts <= total
    b = np.sort(rng.choice(np.arange(1, total), parts - 1, replace=False)) if parts > 1 else np.zeros(0, int)
    lens = np.diff(np.concatenate([[0], b, [total]])).astype(np.int64)
    assert lens.min() >= 1 and lens.sum() == total
    return lens


def intervals(lens):
    en = np.cumsum(lens) - 1
    return (en - lens + 1).astype(np.int32), en.astype(np.int32)


def tdu_segments(T, gs, ge, kind, rng):
    """TDU intervals (starts, ends): ``one`` segment, ``frames`` (S = T, all of length 1) or ``rand``:
    about T / 5 segments whose boundaries avoid the shortest ground-truth segment (it then lies inside
    one TDU segment), so that some TDU segments span several ground-truth segments."""
    if kind == "one":
        return intervals(np.array([T]))
    if kind == "frames":
        return intervals(np.ones(T, dtype=np.int64))
    S = max(2, T // 5)
    b = set(rng.choice(np.arange(1, T), S - 1, replace=False).tolist())
    k = int(np.argmin(ge - gs))
    for f in range(int(gs[k]), int(ge[k]) + 2):      # a boundary at f separates frames f - 1 and f
        b.discard(f)
    b = np.array(sorted(b), dtype=np.int64)
    return intervals(np.diff(np.concatenate([[0], b, [T]])))


def match_case(T, Q, G, V, N, A, seed, structured=False):
    """Token heads (Q, V + N + 2) fp32, ground-truth segments, and a (T, Q) fp32 score table the
    attention of any segmentation is made from.  ``structured``: token s % Q is boosted for segment s in
    both the heads and the scores (a matching without near-ties)."""
    rng = np.random.default_rng(seed)
    vids, nids = mapping(V, N, A, seed=A)
    gs, ge = intervals(cuts(T, G, rng))
    gl = rng.integers(0, A, G).astype(np.int32)
    gl[-1] = A - 1
    acl = rng.standard_normal((Q, V + N + 2)) * (0.5 if structured else 2.0)
    score = rng.standard_normal((T, Q)) * (0.3 if structured else 2.0)
    if structured:
        tok = np.arange(G) % Q
        if G > Q:                                  # o2m: all segments of an action share its token
            tok = gl % Q
        for s in range(G):
            q = int(tok[s])
            score[gs[s]:ge[s] + 1, q] += 4.0 + 0.5 * ((s * 7) % 5)
            acl[q, vids[gl[s]]] += 8.0
            acl[q, V + 1 + nids[gl[s]]] += 8.0
    return dict(T=T, Q=Q, G=G, V=V, N=N, A=A, vids=vids, nids=nids, gs=gs, ge=ge, gl=gl,
                acl=torch.from_numpy(acl).float(), score=torch.from_numpy(score).float())


def seg_attention(case, st, en, zero_token=None):
    """(S, Q) fp32 segment attention (softmax over the tokens of the mean score of each TDU segment; one
    token zeroed everywhere on request) and its (T, Q) frame-level gather."""
    sc = case["score"]
    rows = torch.stack([sc[int(a):int(b) + 1].mean(0) for a, b in zip(st, en)])
    attn = torch.softmax(rows, -1)
    if zero_token is not None:
        attn[:, zero_token] = 0.0
    seg_id = torch.repeat_interleave(torch.arange(len(st)), torch.from_numpy((en - st + 1).astype(np.int64)))
    return attn.contiguous(), attn[seg_id].contiguous()


def ref_cost(case, attn_frame, pc, a2fc, dtype=torch.float64, device="cpu"):
    """MatchCriterion.match's cost (loss.py:108-153) with a2f_soft_iou's cube (loss.py:91-106) and the
    token probabilities exp(action_logp) of blocks_SepVerbNoun.py:189-224."""
    a = attn_frame.to(device=device, dtype=dtype)                           # (T, Q)
    T, Q = a.shape
    G = case["G"]
    gs, ge = case["gs"], case["ge"]
    seg_label = torch.repeat_interleave(torch.arange(G), torch.from_numpy((ge - gs + 1).astype(np.int64)))
    onehot = torch.nn.functional.one_hot(seg_label, G).to(device=device, dtype=dtype)   # (T, G)
    lp = ref_logp(case["acl"].to(device=device, dtype=dtype), case["vids"], case["nids"], case["V"] + 1, True)
    prob = torch.exp(lp)
    cost = torch.zeros(Q, G, dtype=dtype, device=device)
    if pc > 0:
        cost = cost - pc * prob[:, torch.from_numpy(case["gl"].astype(np.int64)).to(device)]
    if a2fc > 0:
        overlap = a.t() @ onehot
        union = torch.minimum(a[:, :, None] + onehot[:, None, :], torch.ones((), dtype=dtype, device=device)).sum(0)
        cost = cost - a2fc * torch.nan_to_num(overlap / union, nan=0.0)
    return cost


def matches(cost, gl):
    """(o2o pairs, o2m pairs) of a host float64 cost matrix."""
    c = np.asarray(cost, dtype=np.float64)
    ai, si = linear_sum_assignment(c)
    am, sm = one_to_many_match(c, np.asarray(gl))
    return (ai.tolist(), si.tolist()), (list(map(int, am)), list(map(int, sm)))


def match_is_stable(cost64, gl, bound):
    """The matches of cost64 and of cost64 moved by +-bound in two seeded sign patterns are the same."""
    c = cost64.cpu().numpy()
    want = matches(c, gl)
    for seed in (1, 2):
        sign = np.where(np.random.default_rng(seed).random(c.shape) < 0.5, -1.0, 1.0)
        if matches(c + bound * sign, gl) != want:
            return False
    return True
