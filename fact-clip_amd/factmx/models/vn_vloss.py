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

The lockstep batch (blocks_SepVerbNoun.LOCKSTEP) takes ``run_batch``: the last block launches
functional.vn_match_cost_batch for every video and reads the costs back through pinned memory while the
forward goes on (``BatchMatch``); after the host matching ONE table holds the terms above of every block of
every video (``batch_plan``: [batch loss, per-video loss, per-video per-block values]), then
functional.vn_eval_pred_batch and one read-back of predictions, loss values and the status word.
"""
import ctypes

import numpy as np
import torch

from .. import functional as fxf
from .. import native as nx
from .vloss import (EarlyMatch, TableTooLarge, _LossFn, _Pack, _contig_strides, _pinned, class_weights, gt_segments,
                    segment_weights)

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


# ---------------------------------------------------------------------------
# The lockstep batch (blocks_SepVerbNoun.LOCKSTEP): one matching-cost launch, one term table, one
# prediction pass and one read-back for every video of the step
# ---------------------------------------------------------------------------

def batch_plan(kinds, Ts, S, Q, A, sw):
    """``term_plan`` for every video of a batch.  ``S[k][v]``: TDU segments of block k in video v.
    Returns per term (video, block, name, c_ce, c_sm) -- video-major, each video's terms in
    ``term_plan``'s order -- and the (1 + nvid + nvid * blocks) x terms coefficient matrix of
    [batch loss, per-video loss, per-video per-block values]: the reference's mean over videos of the
    mean over blocks."""
    nvid, nb = len(Ts), len(kinds)
    rows, per = [], []
    for v, T in enumerate(Ts):
        r, c = term_plan(kinds, T, [S[k][v] for k in range(nb)], Q, A, sw)
        rows.extend((v,) + x for x in r)
        per.append(c)
    coef = np.zeros((1 + nvid + nvid * nb, len(rows)), dtype=np.float32)
    i = 0
    for v, c in enumerate(per):
        n = c.shape[1]
        coef[0, i:i + n] = c[0] / nvid
        coef[1 + v, i:i + n] = c[0]
        coef[1 + nvid + v * nb:1 + nvid + (v + 1) * nb, i:i + n] = c[1:]
        i += n
    return rows, coef


def _i32_view(pk, off, n):
    return pk.dev[off:off + 4 * n].view(torch.int32)


class BatchMatch(EarlyMatch):
    """vloss.EarlyMatch for the verb/noun batch: the last block calls it as soon as its token logits and
    token -> segment attention exist (before sf_merge and its frame branch): ONE
    functional.vn_match_cost_batch launch for every video and an asynchronous pinned read-back of the
    costs, so the host matching (``matches``, inherited) overlaps the rest of the forward."""

    def prepare(self, dev):
        """The label-only host work: ground-truth segments, int32 labels and class weights in one upload
        (the first TDU block runs it while the host waits for its segment counts)."""
        if self.prepared:
            return
        net = self.net
        gts, labs = [], []
        for lh, ev in self.hosts:
            if ev is not None:
                ev.synchronize()
            lab = lh.numpy() if torch.is_tensor(lh) else np.asarray(lh)
            labs.append(lab)
            gts.append(gt_segments(lab))
        G = [len(g[0]) for g in gts]
        pk = _Pack()
        gt_off = [tuple(pk.array(a, np.int32) for a in g) for g in gts]
        lab_off = [pk.array(lab, np.int32) for lab in labs]
        cw = class_weights(net.mcriterion, net.vnmap.num_actions + 1)
        cw_off = pk.array(cw, np.float32)
        base = pk.alloc(dev)
        pk.send()
        self.__dict__.update(labs=labs, gts=gts, G=G, Gmax=max(G), gt_off=gt_off, lab_off=lab_off, cw=cw,
                             cw_off=cw_off, pk=pk, base=base)
        self.prepared = True

    def __call__(self, vb, a_cl, a2f_at, seg):
        cfg = self.net.cfg
        dev = a_cl.device
        self.prepare(dev)
        self.cost_host = None
        if cfg.Loss.match != "seq":
            s_off, local = seg
            Q = vb.Q
            ac = vb.tokens(a_cl)
            at = torch.split(a2f_at.detach(), [Q * (s_off[v + 1] - s_off[v]) for v in range(vb.nvid)])
            videos = []
            for v in range(vb.nvid):
                gs, ge, gl = (_i32_view(self.pk, o, self.G[v]) for o in self.gt_off[v])
                videos.append(dict(action_clogit=ac[v], attn=at[v].view(-1, Q), seg_start=local[v][1],
                                   seg_end=local[v][2], gs=gs, ge=ge, gl=gl, T=vb.Ts[v]))
            pc, a2fc = float(cfg.Loss.pc), float(cfg.Loss.a2fc)
            with torch.no_grad():
                cost = fxf.vn_match_cost_batch(videos, self.net.vnmap, pc if pc > 0 else 0.0,
                                               a2fc if a2fc > 0 else 0.0)
            self.cost_host = _pinned("vn_cost", cost.shape, torch.float32)
            self.cost_host.copy_(cost, non_blocking=True)
            self.cost_ready = torch.cuda.Event()
            self.cost_ready.record()
            self.cost_dev = cost
        self.done = True


def _pred_videos(net, vb):
    last = net.block_list[-1]._bt
    Q = vb.Q
    s_off, local = last["s_off"], last["local"]
    ac, fc = vb.tokens(last["a_cl"]), vb.frames(last["f_cl"])
    at = torch.split(last["a2f_at"].detach(), [Q * (s_off[v + 1] - s_off[v]) for v in range(vb.nvid)])
    return [dict(action_clogit=ac[v], frame_clogit=fc[v], attn=at[v].view(-1, Q), seg_id=local[v][0])
            for v in range(vb.nvid)]


def run_batch(net, vb, compute_loss, early=None):
    """Predictions (and with ``compute_loss`` the batch loss and the per-video loss values) of the lockstep
    batch whose stacked block outputs ``forward_batch`` left in ``blk._bt``.  After the matching ONE term
    table holds every term of every block of every video (one upload, one fx_loss_terms_fwd, one autograd
    node, one fx_loss_terms_bwd); then functional.vn_eval_pred_batch and ONE read-back of the predictions,
    the loss values and the status word.  Returns FACT.forward's value: save_list, or (loss, save_list).
    Raises vloss.TableTooLarge, with nothing but the costs launched, when a video's match pairs more than
    FX_LOSS_MAXK columns."""
    lib = nx.load()
    cfg = net.cfg
    blocks = list(net.block_list)
    vnmap = net.vnmap
    A, V, N = vnmap.num_actions, vnmap.num_verbs, vnmap.num_nouns
    nvid, Q, Ts, fo = vb.nvid, vb.Q, vb.Ts, vb.f_off
    nb = len(blocks)
    dev = blocks[-1]._bt["f_cl"].device
    out = loss = None
    if compute_loss:
        assert early is not None and early.done, "the last block did not run the early matching stage"
        crit = net.mcriterion
        matches = early.matches(Q)
        net.__dict__["_matches"] = matches         # per video (token indices, segment indices), host int64
        mts = [match_tables(crit, early.gts[v], matches[v], Q, A, early.cw) for v in range(nvid)]
        big = [v for v, mt in enumerate(mts) if mt is None]
        if big:
            raise TableTooLarge(big)
        kinds = ["U" if hasattr(blk, "a2f_layer") else "I" for blk in blocks]
        rows, coef = batch_plan(kinds, Ts, [blk._bt["S"] for blk in blocks], Q, A, float(cfg.Loss.sw))
        nterms, nout = len(rows), coef.shape[0]

        # every differentiated input (the blocks' stacked logits), its gradient a view of ONE flat allocation
        inputs = []
        for blk, letter in zip(blocks, kinds):
            bt = blk._bt
            inputs.extend((bt["f_cl"], bt["seg_cl"], bt["a_cl"]))
            if letter == "U":
                inputs.extend((bt["f2a_lg"], bt["a2f_lg"]))
        sizes = [(t.numel() + 63) & ~63 for t in inputs]
        goff = [0]
        for n_ in sizes[:-1]:
            goff.append(goff[-1] + n_)
        gflat = torch.empty(sum(sizes), device=dev, dtype=torch.float32)
        gaddr = {id(t): gflat.data_ptr() + 4 * o for t, o in zip(inputs, goff)}

        pk = _Pack()
        o_tgt = [pk.array(mt["tgt"], np.int32) for mt in mts]
        o_k = [[pk.array(mt[n_], dt) for n_, dt in (("ka", np.int32), ("kgs", np.int32), ("kge", np.int32),
                                                     ("ksw", np.float32))] for mt in mts]
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
        cw_p = early.base + early.cw_off

        slots = []
        for i, (v, k, name, c_ce, c_sm) in enumerate(rows):
            bt = blocks[k]._bt
            t = terms[i]
            t.slot, t.c_ce, t.c_sm = i, c_ce, c_sm
            Sv, s0 = bt["S"][v], bt["s_off"][v]
            rs, re = bt["local"][v][1].data_ptr(), bt["local"][v][2].data_ptr()
            if name in ("frame", "seg", "token"):
                x = bt[{"frame": "f_cl", "seg": "seg_cl", "token": "a_cl"}[name]]
                row0, R = {"frame": (fo[v], Ts[v]), "seg": (s0, Sv), "token": (v * Q, Q)}[name]
                C, ldx = int(x.shape[1]), nx.ld(x)
                j = 1 if name == "token" else 0
                t.kind, t.R, t.C = nx.TERM_VNCLASS, R, C
                t.x, t.sr, t.sc = x.data_ptr() + 4 * row0 * ldx, ldx, 1
                t.dx, t.dsr, t.dsc = gaddr[id(x)] + 4 * row0 * C, C, 1
                t.w, t.vn, t.vn_host = cw_p, vn_dev[j], vn_host[j]
                if name == "token":
                    t.y = base + o_tgt[v]
                else:
                    t.y = early.base + early.lab_off[v]
                    if name == "seg":
                        t.rs, t.re, t.D = rs, re, Ts[v]
                slots.append((2 * R, 0, 0))
            else:
                # video v's f2a logits (Q, S_v) read as (S_v, Q): log_softmax over the rows of each matched
                # column (axis 0); its a2f logits (S_v, Q): log_softmax over the matched columns of each row
                L = bt["f2a_lg" if name == "f2a" else "a2f_lg"]
                if L.numel() != Q * bt["s_off"][-1]:
                    raise RuntimeError(f"vn_vloss: {name} logits {tuple(L.shape)} for {bt['s_off'][-1]} segments "
                                       f"x {Q} tokens")
                K = mts[v]["K"]
                sr, sc = (1, Sv) if name == "f2a" else (Q, 1)
                t.kind, t.R, t.C, t.axis, t.K = nx.TERM_ATTN, Sv, Q, (0 if name == "f2a" else 1), K
                t.x, t.sr, t.sc = L.data_ptr() + 4 * Q * s0, sr, sc
                t.dx, t.dsr, t.dsc = gaddr[id(L)] + 4 * Q * s0, sr, sc
                t.rs, t.re = rs, re
                t.ka, t.kgs, t.kge, t.ksw = (base + o for o in o_k[v])
                slots.append((Sv, Sv + K, K))
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
                    keep=(early, pk, scr, vids, nids, [blk._bt for blk in blocks], inputs))
        out, loss = _LossFn.apply(plan, *inputs)
        o = 1 + nvid + (nvid - 1) * nb
        net.loss_list = [out[o + k] for k in range(nb)]        # the last video's per-block values

    pred = fxf.vn_eval_pred_batch(_pred_videos(net, vb), vnmap, cfg.FACT.mwt)
    parts = [pred.to(torch.float64)]
    if compute_loss:
        parts.append(out.detach().to(torch.float64))
    parts.append(fxf.device_status(dev)[:1].to(torch.float64))
    host = torch.cat(parts).cpu().numpy()              # the step's one read-back
    fxf.status_raise(int(host[-1]), dev)
    saves = [{"pred": host[fo[v]:fo[v + 1]].astype("int64")} for v in range(nvid)]
    if not compute_loss:
        return saves
    for v, save in enumerate(saves):
        save["loss"] = {"loss": float(host[fo[-1] + 1 + v])}
    return loss, saves
