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
  fx_loss_terms_bwd  every logit tensor's gradient in one autograd node (termtable._LossFn).

A video whose match pairs more than FX_LOSS_MAXK columns, or a model with ``cfg.FACT.trans``, takes
the per-term path of Block.compute_loss.

The lockstep batch (blocks_SepVerbNoun.LOCKSTEP) takes ``run_batch``: the last block launches
functional.vn_match_cost_batch for every video and reads the costs back through pinned memory while the
forward goes on (``BatchMatch``); after the host matching ONE table holds the terms above of every block of
every video (``batch_plan``: [batch loss, per-video loss, per-video per-block values]), then
functional.vn_eval_pred_batch and one read-back of predictions, loss values and the status word.

``run`` and ``run_batch`` share ``_launch`` / ``_fill`` on models/termtable.TermTable and differ only in where a
term's rows live: ``_sources`` (the blocks' own tensors, a batch of one) or ``_batch_sources`` (the stacked ``_bt``).
"""
import collections

import numpy as np
import torch

from .. import functional as fxf
from .. import native as nx
from .termtable import TermTable, _Pack
from .vloss import EarlyMatch, TableTooLarge, _pinned, class_weights, gt_segments, segment_weights

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


# ---------------------------------------------------------------------------
# The table of one video or of a batch: where each term's rows live, and the one loop that fills it
# ---------------------------------------------------------------------------

# One term's rows: ``t`` the differentiated input, ``x`` the tensor the kernel reads (``t`` or a view of it),
# ``xoff`` / ``goff`` the element offset of the video's first row in ``x`` and in ``t``'s gradient, R x C rows
# with the element strides ``sr`` / ``sc`` of ``x`` and ``dsr`` / ``dsc`` of the (contiguous) gradient.
_Src = collections.namedtuple("_Src", "t x xoff goff R C sr sc dsr dsc")
# One block of one video: class terms, attention terms (None: an input block), its TDU intervals' addresses.
_Blk = collections.namedtuple("_Blk", "frame seg token f2a a2f rs re")
# One video: frames, matched columns, the addresses of its int32 labels, token targets and (ka, kgs, kge, ksw).
_Vid = collections.namedtuple("_Vid", "T K lab tgt kcols")
_KCOLS = (("ka", np.int32), ("kgs", np.int32), ("kge", np.int32), ("ksw", np.float32))


def _class_src(t, x, row0, R, C, ldx):
    """Rows ``row0 .. row0 + R`` of the (rows, C) class logits ``x`` of row stride ``ldx``."""
    return _Src(t, x, row0 * ldx, row0 * C, R, C, ldx, 1, C, 1)


def _attn_src(name, L, off, shape, st, S, Q):
    """A video's attention logits read as (S, Q): its (Q, S) [f2a: log_softmax over the rows of each matched
    column, axis 0] or (S, Q) [a2f: over the matched columns of each row, axis 1] block of ``shape`` and
    element strides ``st`` at element ``off`` of the input ``L``; its gradient block is contiguous."""
    if tuple(shape) != ((Q, S) if name == "f2a" else (S, Q)):
        raise RuntimeError(f"vn_vloss: {name} logits {tuple(shape)} of {tuple(L.shape)} for {S} segments x {Q} tokens")
    if name == "f2a":
        return _Src(L, L, off, off, S, Q, st[1], st[0], 1, S)
    return _Src(L, L, off, off, S, Q, st[0], st[1], Q, 1)


def _sources(blocks, kinds, S, Q):
    """``src[0][block]`` of one video from the blocks' own tensors: (R, 1, C) class logits, (1, Q, S) /
    (1, S, Q) attention logits and the TDU's intervals -- a batch of one video."""
    out = []
    for blk, letter, Sk in zip(blocks, kinds, S):
        cl = [_class_src(x3, x, 0, int(x.shape[0]), int(x.shape[1]), nx.ld(x))
              for x3, x in ((x3, fxf._2d(x3)) for x3 in blk._clogits)]
        at = [None, None]
        if letter == "U":
            at = [_attn_src(n_, L3, 0, L3.shape[1:], L3.stride()[1:], Sk, Q)
                  for n_, L3 in (("f2a", blk.f2a_attn_logit), ("a2f", blk.a2f_attn_logit))]
        out.append(_Blk(*cl, *at, blk.tdu.start32.data_ptr(), blk.tdu.end32.data_ptr()))
    return [out]


def _batch_sources(bts, kinds, Ts, fo, Q):
    """``src[video][block]`` from the blocks' stacked ``_bt`` tensors: video v's frame rows at ``fo[v]``,
    segment rows at ``s_off[v]``, token rows at ``v * Q``, and its (Q, S_v) / (S_v, Q) attention block at
    element ``Q * s_off[v]`` of the logits (every video's block back to back, the element step the tensor's)."""
    out = [[] for _ in Ts]
    for bt, letter in zip(bts, kinds):
        S, s_off = bt["S"], bt["s_off"]
        if letter == "U":
            Lf, La = bt["f2a_lg"], bt["a2f_lg"]
            for n_, L in (("f2a", Lf), ("a2f", La)):
                if L.numel() != Q * s_off[-1]:
                    raise RuntimeError(f"vn_vloss: {n_} logits {tuple(L.shape)} for {s_off[-1]} segments x {Q} tokens")
            ef, ea = Lf.view(-1).stride(0), La.view(-1).stride(0)
        (f, fC, fld), (s, sC, sld), (a, aC, ald) = ((x, int(x.shape[1]), nx.ld(x))
                                                    for x in (bt["f_cl"], bt["seg_cl"], bt["a_cl"]))
        for v, T in enumerate(Ts):
            Sv, s0 = S[v], s_off[v]
            at = [None, None]
            if letter == "U":
                at = [_attn_src("f2a", Lf, Q * s0 * ef, (Q, Sv), (Sv * ef, ef), Sv, Q),
                      _attn_src("a2f", La, Q * s0 * ea, (Sv, Q), (Q * ea, ea), Sv, Q)]
            out[v].append(_Blk(_class_src(f, f, fo[v], T, fC, fld), _class_src(s, s, s0, Sv, sC, sld),
                               _class_src(a, a, v * Q, Q, aC, ald), *at,
                               bt["local"][v][1].data_ptr(), bt["local"][v][2].data_ptr()))
    return out


def _inputs(src):
    """Every differentiated input of the sources, block by block (TermTable drops the repeats)."""
    return [s.t for blks in src for b in blks for s in b[:5] if s is not None]


def _fill(tt, rows, src, vids, w, vn):
    """Every term of ``rows`` ((video, block, name, c_ce, c_sm)) in order -- the kernels' summation order --
    from ``src[video][block]`` and the per-video ``vids``, then the scratch layout.  ``w``: the class weights'
    address, ``vn``: TermTable.vn_pair's two mappings."""
    for v, k, name, c_ce, c_sm in rows:
        b, pv = src[v][k], vids[v]
        s = getattr(b, name)
        x = s.x.data_ptr() + 4 * s.xoff
        if name in ("f2a", "a2f"):
            t = tt.add(nx.TERM_ATTN, s.R, s.C, x, s.sr, s.sc, s.t, s.goff, s.dsr, s.dsc, c_ce, c_sm, pv.K)
            t.axis, t.K, t.rs, t.re = (0 if name == "f2a" else 1), pv.K, b.rs, b.re
            t.ka, t.kgs, t.kge, t.ksw = pv.kcols
        else:
            t = tt.add(nx.TERM_VNCLASS, s.R, s.C, x, s.sr, s.sc, s.t, s.goff, s.dsr, s.dsc, c_ce, c_sm)
            t.w = w
            t.vn, t.vn_host = vn[1 if name == "token" else 0]
            if name == "token":
                t.y = pv.tgt
            else:
                t.y = pv.lab
                if name == "seg":
                    t.rs, t.re, t.D = b.rs, b.re, pv.T
    tt.lay_out()


def _launch(pk, dev, rows, coef, src, mts, Ts, lab, w, vnmap, keep):
    """The table of ``rows`` on the pack ``pk`` (the caller's own arrays reserved), sent and run: (out, loss).
    ``mts[v]``: video v's match tables; ``lab[v]`` / ``w``: (pack, offset) of its int32 labels / of the class
    weights -- ``pk`` itself or a pack sent earlier."""
    o_tgt = [pk.array(mt["tgt"], np.int32) for mt in mts]
    o_k = [[pk.array(mt[n_], dt) for n_, dt in _KCOLS] for mt in mts]
    tt = TermTable(pk, dev, _inputs(src), coef, nvn=2)
    base = tt.base
    vids = [_Vid(Ts[v], mt["K"], lab[v][0].base + lab[v][1], base + o_tgt[v], [base + o for o in o_k[v]])
            for v, mt in enumerate(mts)]
    _fill(tt, rows, src, vids, w[0].base + w[1], tt.vn_pair(vnmap))
    tt.send()
    return tt.launch(keep=(src, keep))


def run(net, crit, match, label):
    """The video loss of the blocks' saved class logits and attention logits for ``match``; sets
    ``net.loss_list`` (views of the table's per-block outputs).  None: the match is too large for the
    table, nothing was launched."""
    blocks = list(net.block_list)
    A = net.vnmap.num_actions
    f0 = blocks[0]._clogits[0]
    T, Q = int(f0.shape[0]), int(blocks[0]._clogits[2].shape[0])
    lab = _host_labels(crit, label)
    gts = gt_segments(lab)
    cw = class_weights(crit, A + 1)
    mt = match_tables(crit, gts, match, Q, A, cw)
    if mt is None:
        return None
    kinds = ["U" if hasattr(blk, "a2f_layer") else "I" for blk in blocks]
    S = [int(blk.tdu.num_seg) for blk in blocks]
    rows, coef = term_plan(kinds, T, S, Q, A, float(net.cfg.Loss.sw))
    pk = _Pack()                               # (the labels and the class weights travel with the table)
    o_lab, o_cw = pk.array(lab, np.int32), pk.array(cw, np.float32)
    out, loss = _launch(pk, f0.device, [(0,) + r for r in rows], coef, _sources(blocks, kinds, S, Q), [mt], [T],
                        [(pk, o_lab)], (pk, o_cw), net.vnmap, [blk.tdu for blk in blocks])
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
    cfg = net.cfg
    blocks = list(net.block_list)
    vnmap = net.vnmap
    A = vnmap.num_actions
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
        bts = [blk._bt for blk in blocks]
        rows, coef = batch_plan(kinds, Ts, [bt["S"] for bt in bts], Q, A, float(cfg.Loss.sw))
        lab, w = [(early.pk, o) for o in early.lab_off], (early.pk, early.cw_off)
        out, loss = _launch(_Pack(), dev, rows, coef, _batch_sources(bts, kinds, Ts, fo, Q), mts, Ts, lab, w, vnmap,
                            (early, bts))
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
