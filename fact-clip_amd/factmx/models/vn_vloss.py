"""The loss phase of one video of the verb/noun FACT (models/blocks_SepVerbNoun.py) from one
device-resident term table, as models/vloss.py does for the lockstep batch of models/blocks.py.

The reference computes, per block, frame_loss / frame_loss_tdu / smooth_loss / action_token_loss on the
materialised action log-probabilities and, per update block, two cross_attn_loss_tdu terms on "zoomed"
one-hot tables (blocks_SepVerbNoun.py:298-321, 487-496 over loss.py:195-277).  Here, after the matching
(MatchCriterion.match: fx_vn_match_cost, the host Hungarian), ONE upload of the table and

  fx_loss_terms_fwd  per block a frame term (FX_TERM_VNCLASS: 0.25/T, smooth sw/((T-1)A)), a segment
                     term (FX_TERM_VNCLASS with the TDU intervals over the frame labels: 0.25/S) and a
                     token term (FX_TERM_VNCLASS with null column, targets from the match: 0.5/Q); per
                     update block the f2a (axis 0) and a2f (axis 1) terms (FX_TERM_ATTN with interval
                     targets, 1/S); the coefficient matrix gives [video loss, per-block values]
  fx_loss_terms_bwd  every logit tensor's gradient in one autograd node (vloss._LossFn).

A video whose match pairs more than FX_LOSS_MAXK columns, or a model with ``cfg.FACT.trans``, takes
the per-term path of Block.compute_loss.
"""
import ctypes

import numpy as np
import torch

from .. import functional as fxf
from .. import native as nx
from .vloss import _Pack, _LossFn, _contig_strides, gt_segments, class_weights, segment_weights

# The loss terms of a video of CUDA inputs from one term table (with blocks_SepVerbNoun.FUSED_LOSS);
# False: one launch pair per class term and the eager cross-attention terms.
FUSED_TABLE = True


def supported(net):
    """The table covers a model without transcripts whose blocks kept their class logits on the device
    (FUSED_LOSS on CUDA inputs) and whose last block is an update block (the matching reads its
    token -> segment attention)."""
    last = net.block_list[-1]
    if net.cfg.FACT.trans or net.cfg.Loss.match not in ("o2o", "o2m", "seq"):
        return False
    if getattr(last, "a2f_seg_attn", None) is None:
        return False
    return all(getattr(blk, "_fused", False) for blk in net.block_list)


def match_tables(crit, gts, match, Q, A, cw):
    """What the table takes from the match (host arrays): the token targets (Q) int32 -- a matched token
    its segment's action, every other token the null column A --, the matched columns ``ka`` with
    their ground-truth intervals ``kgs`` / ``kge`` and weights ``ksw`` (K each; loss.py:218-219 scales
    column i by sweight[i]), or None when K exceeds FX_LOSS_MAXK."""
    ai = np.asarray(match[0], dtype=np.int64)
    si = np.asarray(match[1], dtype=np.int64)
    K = len(ai)
    if K > nx.LOSS_MAXK:
        return None
    tgt = np.full(Q, A, dtype=np.int32)
    tgt[ai] = gts[2][si]
    swn = segment_weights(crit, gts[2])
    if len(swn) not in (K, 1):
        raise RuntimeError(f"cross_attn_loss: {K} matched columns vs {len(swn)} segment weights")
    ksw = np.empty(K, dtype=np.float32)
    ksw[:] = swn if len(swn) == K else swn[0]
    return dict(K=K, tgt=tgt, ka=ai.astype(np.int32), kgs=gts[0][si].astype(np.int32),
                kge=gts[1][si].astype(np.int32), ksw=ksw)


def term_plan(kinds, T, S, Q, A, sw):
    """The table's layout for blocks of the given letters: per term (block, name, c_ce, c_sm), and the
    (1 + blocks) x terms coefficient matrix of [video loss, per-block values].  ``S[k]``: TDU segments
    of block k."""
    nb = len(kinds)
    rows = []
    for k, letter in enumerate(kinds):
        rows.append((k, "frame", 0.25 / T, (sw / ((T - 1) * A) if sw and T > 1 else 0.0)))
        rows.append((k, "seg", 0.25 / S[k], 0.0))
        rows.append((k, "token", 0.5 / Q, 0.0))
        if letter == "U":
            rows.append((k, "f2a", 1.0 / S[k], 0.0))
            rows.append((k, "a2f", 1.0 / S[k], 0.0))
    coef = np.zeros((1 + nb, len(rows)), dtype=np.float32)
    for i, (k, _, _, _) in enumerate(rows):
        coef[0, i] = 1.0 / nb
        coef[1 + k, i] = 1.0
    return rows, coef


def _host_labels(crit, label):
    lab = getattr(crit, "_label_np", None)
    if lab is None:                      # (after the matching's read-back: the stream is drained already)
        lab = crit._label_np = label.cpu().numpy()
    return np.asarray(lab)


def run(net, crit, match, label):
    """The video loss of the blocks' saved class logits and attention logits for ``match``; sets
    ``net.loss_list`` (views of the table's per-block outputs).  None: the match is too large for the
    table, nothing was launched."""
    lib = nx.load()
    cfg = net.cfg
    blocks = list(net.block_list)
    vnmap = net.vnmap
    A, V, N = vnmap.num_actions, vnmap.num_verbs, vnmap.num_nouns
    f0 = blocks[0]._clogits[0]
    dev = f0.device
    T, Q = int(f0.shape[0]), int(blocks[0]._clogits[2].shape[0])
    lab = _host_labels(crit, label)
    gts = gt_segments(lab)
    cw = class_weights(crit, A + 1)
    mt = match_tables(crit, gts, match, Q, A, cw)
    if mt is None:
        return None
    K = mt["K"]
    kinds = ["U" if hasattr(blk, "a2f_layer") else "I" for blk in blocks]
    S = [int(blk.tdu.num_seg) for blk in blocks]
    rows, coef = term_plan(kinds, T, S, Q, A, float(cfg.Loss.sw))
    nterms, nout = len(rows), 1 + len(blocks)

    # every differentiated input, its gradient a view of ONE flat allocation
    inputs = []
    for blk, letter in zip(blocks, kinds):
        inputs.extend(blk._clogits)
        if letter == "U":
            inputs.extend((blk.f2a_attn_logit, blk.a2f_attn_logit))
    sizes = [(t.numel() + 63) & ~63 for t in inputs]
    goff = [0]
    for n_ in sizes[:-1]:
        goff.append(goff[-1] + n_)
    gflat = torch.empty(sum(sizes), device=dev, dtype=torch.float32)
    gaddr = {id(t): gflat.data_ptr() + 4 * o for t, o in zip(inputs, goff)}

    pk = _Pack()
    o_lab = pk.array(lab, np.int32)
    o_cw = pk.array(cw, np.float32)
    o_tgt = pk.array(mt["tgt"], np.int32)
    o_k = [pk.array(mt[n_], dt) for n_, dt in (("ka", np.int32), ("kgs", np.int32), ("kge", np.int32),
                                               ("ksw", np.float32))]
    o_coef = pk.array(coef, np.float32)
    o_vn, vnt = pk.structs(nx.VnTerm, 2)
    o_t, terms = pk.structs(nx.LossTerm, nterms)
    base = pk.alloc(dev)
    vids, nids = vnmap.tables(dev)
    for j, (n1, n2, null) in enumerate(((V, N, 0), (V + 1, N + 1, 1))):
        m = vnt[j]
        m.n1, m.n2, m.A, m.null = n1, n2, A, null
        m.vids, m.nids = vids.data_ptr(), nids.data_ptr()
        m.voff, m.vlist, m.noff, m.nlist = (t.data_ptr() for t in vnmap.csr(dev, n1, n2))
    vn_dev = [base + o_vn + j * ctypes.sizeof(nx.VnTerm) for j in range(2)]
    vn_host = [ctypes.addressof(vnt[j]) for j in range(2)]

    slots = []
    for i, (k, name, c_ce, c_sm) in enumerate(rows):
        blk = blocks[k]
        t = terms[i]
        t.slot, t.c_ce, t.c_sm = i, c_ce, c_sm
        if name in ("frame", "seg", "token"):
            x3 = blk._clogits[("frame", "seg", "token").index(name)]
            x = fxf._2d(x3)
            j = 1 if name == "token" else 0
            t.kind, t.R, t.C = nx.TERM_VNCLASS, int(x.shape[0]), int(x.shape[1])
            t.x, t.sr, t.sc = x.data_ptr(), nx.ld(x), 1
            t.dx, t.dsr, t.dsc = gaddr[id(x3)], t.C, 1
            t.w, t.vn, t.vn_host = base + o_cw, vn_dev[j], vn_host[j]
            if name == "token":
                t.y = base + o_tgt
            else:
                t.y = base + o_lab
                if name == "seg":
                    t.rs, t.re, t.D = blk.tdu.start32.data_ptr(), blk.tdu.end32.data_ptr(), T
            slots.append((2 * t.R, 0, 0))
        else:
            # f2a logits (1, Q, S) read as (S, Q): log_softmax over the rows of each matched column (axis 0);
            # a2f logits (1, S, Q): log_softmax over the matched columns of each row (axis 1)
            L3 = blk.f2a_attn_logit if name == "f2a" else blk.a2f_attn_logit
            L = L3[0].t() if name == "f2a" else L3[0]
            R, C = int(L.shape[0]), int(L.shape[1])
            if (R, C) != (S[k], Q):
                raise RuntimeError(f"vn_vloss: {name} logits {tuple(L3.shape)} for {S[k]} segments x {Q} tokens")
            d3 = _contig_strides(L3.shape)
            t.kind, t.R, t.C, t.axis, t.K = nx.TERM_ATTN, R, C, (0 if name == "f2a" else 1), K
            t.x, t.sr, t.sc = L.data_ptr(), L.stride(0), L.stride(1)
            t.dx = gaddr[id(L3)]
            t.dsr, t.dsc = (d3[2], d3[1]) if name == "f2a" else (d3[1], d3[2])
            t.rs, t.re = blk.tdu.start32.data_ptr(), blk.tdu.end32.data_ptr()
            t.ka, t.kgs, t.kge, t.ksw = (base + o for o in o_k)
            slots.append((R, R + K, K))
    sc_, offs = 0, []
    for sz in slots:
        o3 = []
        for n_ in sz:
            o3.append(sc_)
            sc_ += (max(n_, 1) + 3) & ~3
        offs.append(o3)
    scr = torch.empty(sc_, device=dev, dtype=torch.float32)
    for t, o3 in zip(terms, offs):
        t.lse, t.lse2, t.colz = (scr.data_ptr() + 4 * o for o in o3)
    ws = torch.empty(max(lib.fx_loss_terms_workspace_floats(nterms), 1), device=dev, dtype=torch.float32)
    pk.send()
    plan = dict(terms_host=terms, terms_dev=base + o_t, nterms=nterms, coef_dev=base + o_coef, nout=nout, ws=ws,
                grads=(gflat, goff, [(t.shape, _contig_strides(t.shape)) for t in inputs]),
                keep=(pk, scr, vids, nids, [blk.tdu for blk in blocks], inputs))   # (the backward reads the logits)
    out, loss = _LossFn.apply(plan, *inputs)
    net.loss_list = [out[1 + k] for k in range(len(blocks))]
    return loss
