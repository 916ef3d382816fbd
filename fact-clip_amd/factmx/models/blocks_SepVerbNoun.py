"""The EPIC-Kitchens FACT with separate verb / noun class heads, with the reference's Python
surface (fact_clip/models/blocks_SepVerbNoun.py).

Same constructor, sub-module creation order, parameter names and shapes, block letters (``I``:
InputBlockTDU, ``U``: UpdateBlockTDU) and side-channel attributes (``frame_logp``, ``seg_logp``,
``action_logp``, ``tdu``, ``f2a_attn(_logit)``, ``a2f_attn(_logit)``).  Every action
log-probability is ``log_softmax(verb)[VIDS[a]] + log_softmax(noun)[NIDS[a]]``; the action ->
(verb, noun) tables live in a ``functional.VerbNounMap`` (the reference's module globals ``_VIDS`` /
``_NIDS``), installed by ``init_VIDS_NIDS`` / ``set_verb_noun_ids`` / ``load_verb_noun_ids`` and
captured by a model at construction.  Compute runs on the HIP kernels through factmx.functional;
videos run one by one and the losses per video, as in the reference, unless ``LOCKSTEP`` is on (below).
With ``FUSED_LOSS`` the class terms of the loss and the prediction of CUDA inputs come straight from
the class logits (functional.vn_class_loss / vn_eval_pred): ``frame_logp`` / ``seg_logp`` are then
computed only when something reads them.  With ``vn_vloss.FUSED_TABLE`` as well, the matching cost comes
from the token heads and the segment-level attention (functional.vn_match_cost) and every loss term of
the video runs from one term table (models/vn_vloss.py); the frame-level ``a2f_attn`` / ``f2a_attn`` are
gathered from the segment rows only when something reads them.  With ``LOCKSTEP`` on top of both, a
batch of CUDA videos (any lengths, at most blocks.MAX_LOCKSTEP_VIDEOS, no ``cfg.FACT.trans``) runs
every block over the stacked videos (``forward_batch``), with one matching-cost launch, one term table,
one prediction pass and one read-back per step (vn_vloss.run_batch); the side-channel attributes then hold
the last video's views, as in models.blocks.
"""
import torch
import torch.nn as nn

from .. import functional as fxf
from ..configs.utils import update_from
from . import basic
from . import blocks
from . import loss
from . import vloss
from . import vn_vloss
from .basic import time_mask, torch_class_label_to_segment_label
from .blocks import _frame_branch_batch, _frame_pos, _Lazy, _lazy_attr, _set_side, _VideoBatch
from .loss import MatchCriterion

_VNMAP = None     # the installed mapping (reference: _VIDS / _NIDS)

# The per-video loss terms and the prediction of CUDA inputs straight from the class logits
# (functional.vn_class_loss / vn_eval_pred: no T x A table of action log-probabilities is built);
# False: the eager forms on the materialised tables.
FUSED_LOSS = True

# All videos of a step through every block in one pass (``forward_batch``), one matching-cost launch, one
# loss term table, one prediction pass and one read-back for the whole batch (vn_vloss.run_batch), when
# ``_lockstep_ok`` holds; False, or a batch the guard refuses: the videos run one by one.
LOCKSTEP = False

MAPPING_FILES = ("./data/epic-kitchens/processed/mapping.txt",
                 "./data/epic-kitchens/processed/verb_mapping.txt",
                 "./data/epic-kitchens/processed/noun_mapping.txt")


def set_verb_noun_ids(vids, nids):
    """Install an action -> (verb id, noun id) mapping directly (lists indexed by action id)."""
    global _VNMAP
    _VNMAP = fxf.VerbNounMap(vids, nids)
    return _VNMAP


def load_verb_noun_ids(mapping, verb_mapping, noun_mapping):
    """blocks_SepVerbNoun.py:154-170 with explicit paths: ``mapping`` lines are ``<id> <verb>,<noun>``,
    the two word files ``<id> <name>``.  Installs and returns the mapping."""
    from ..utils.dataset import load_action_mapping
    v2i, _ = load_action_mapping(verb_mapping)
    n2i, _ = load_action_mapping(noun_mapping)
    vids, nids = [], []
    with open(mapping) as fp:
        lines = fp.read().split("\n")[:-1]
    for line in lines:
        _, aname = line.split(" ")
        v, n = aname.split(",")
        vids.append(v2i[v])
        nids.append(n2i[n])
    return set_verb_noun_ids(vids, nids)


def init_VIDS_NIDS():
    """blocks_SepVerbNoun.py:148-170: read the EPIC-Kitchens mapping files (relative to the working
    directory, as the reference does) unless a mapping is installed already."""
    if _VNMAP is None:
        load_verb_noun_ids(*MAPPING_FILES)
    return _VNMAP


def _lockstep_ok(net, seq_list):
    """The lockstep pass (any video lengths, one video included) needs the fused loss phase with its term
    table, at most blocks.MAX_LOCKSTEP_VIDEOS videos, no transcript input, CUDA inputs and the fused
    decoders; the matching reads the last block's token -> segment attention."""
    if not (FUSED_LOSS and vn_vloss.FUSED_TABLE):
        return False
    if not seq_list or len(seq_list) > blocks.MAX_LOCKSTEP_VIDEOS or net.cfg.FACT.trans:
        return False
    if any(not s.is_cuda or s.shape[0] < 1 for s in seq_list):
        return False
    if net.cfg.Loss.match not in ("o2o", "o2m", "seq") or not hasattr(net.block_list[-1], "a2f_layer"):
        return False
    return all(basic._fused_decoder_ok(blk.action_branch) for blk in net.block_list)


class FACT(nn.Module):
    """blocks_SepVerbNoun.py:14-142."""

    def __init__(self, cfg, in_dim, n_classes1=98, n_classes2=301):
        super().__init__()
        self.vnmap = init_VIDS_NIDS()
        # the reference asserts this on every forward (blocks_SepVerbNoun.py:198-207)
        if (n_classes1, n_classes2) != (self.vnmap.num_verbs, self.vnmap.num_nouns):
            raise ValueError(f"{n_classes1} verb / {n_classes2} noun classes, but the installed mapping has "
                             f"{self.vnmap.num_verbs} / {self.vnmap.num_nouns}")
        self.cfg = cfg
        self.num_classes1 = n_classes1   # verbs
        self.num_classes2 = n_classes2   # nouns
        base_cfg = cfg.Bi
        self.frame_pe = basic.PositionalEncoding(base_cfg.hid_dim, max_len=10000, empty=(not cfg.FACT.fpos))
        self.channel_masking_dropout = nn.Dropout2d(p=cfg.FACT.cmr)
        if not cfg.FACT.trans:
            self.action_query = nn.Parameter(torch.randn([cfg.FACT.ntoken, 1, base_cfg.a_dim]))
        else:
            self.action_pe = basic.PositionalEncoding(base_cfg.a_dim, max_len=1000)
            self.verb_embed = nn.Embedding(n_classes1, base_cfg.a_dim // 2)
            self.noun_embed = nn.Embedding(n_classes2, base_cfg.a_dim // 2)
        block_list = []
        for t in cfg.FACT.block:
            if t == "I":
                block = InputBlockTDU(cfg, in_dim, n_classes1, n_classes2, self.vnmap)
            elif t == "U":
                update_from(cfg.BU, base_cfg, inplace=True)
                base_cfg = cfg.BU
                block = UpdateBlockTDU(cfg, n_classes1, n_classes2, self.vnmap)
            else:
                raise ValueError(t)
            block_list.append(block)
        self.block_list = nn.ModuleList(block_list)
        self.mcriterion = None

    def _forward_one_video(self, seq, transcript=None):
        frame_feature = seq
        frame_pe = _frame_pos(self.frame_pe, seq)
        if self.cfg.FACT.cmr and self.training:
            frame_feature = self.channel_masking_dropout(frame_feature.permute([1, 2, 0])).permute([2, 0, 1])
        if self.cfg.TM.use and self.training:
            frame_feature = time_mask(frame_feature, self.cfg.TM.t, self.cfg.TM.m, self.cfg.TM.p,
                                      replace_with_zero=True)
        if not self.cfg.FACT.trans:
            action_pe = self.action_query
            action_feature = torch.zeros_like(action_pe)
        else:
            vtranscript, ntranscript = self.vnmap.verb_noun_of(transcript)
            action_pe = self.action_pe(transcript)
            vfeature = self.verb_embed(vtranscript).unsqueeze(1)
            nfeature = self.noun_embed(ntranscript).unsqueeze(1)
            action_feature = torch.cat([vfeature, nfeature], dim=-1) + action_pe
            action_pe = torch.zeros_like(action_pe)
        block_output = []
        for block in self.block_list:
            frame_feature, action_feature = block(frame_feature, action_feature, frame_pe, action_pe)
            block_output.append((frame_feature, action_feature))
        return block_output

    def _loss_one_video(self, label):
        mcriterion: MatchCriterion = self.mcriterion
        mcriterion.set_label(label)
        block = self.block_list[-1]
        if vn_vloss.FUSED_TABLE and vn_vloss.supported(self):
            # segment rows + TDU intervals and the token heads: no frame-level attention, no cost cube
            match = mcriterion.match(None, block.a2f_seg_attn, tdu=block.tdu, vn=(block._clogits[2], self.vnmap))
            total = vn_vloss.run(self, mcriterion, match, label)
            if total is not None:
                return total
        else:
            match = mcriterion.match(torch.exp(block.action_logp), block.a2f_attn)
        self.loss_list = [blk.compute_loss(mcriterion, match) for blk in self.block_list]
        return sum(self.loss_list) / len(self.loss_list)

    def _forward_batch(self, seq_list, on_a2f=None):
        """All videos through the blocks in lockstep, as blocks._FACTBase._forward_batch; returns
        restore(v), which points every side-channel attribute at video v's views.  ``on_a2f``
        (vn_vloss.BatchMatch) runs when the last block's token logits and token -> segment attention exist."""
        nvid = len(seq_list)
        vb = _VideoBatch(nvid, [int(s.shape[0]) for s in seq_list], self.cfg.FACT.ntoken)
        vb.on_a2f, vb.last = on_a2f, self.block_list[-1]
        if on_a2f is not None:
            dev = seq_list[0].device
            vb.while_waiting = lambda: on_a2f.prepare(dev)
        frames = []
        for seq in seq_list:
            x = seq.unsqueeze(1)
            if self.cfg.FACT.cmr and self.training:
                x = self.channel_masking_dropout(x.permute([1, 2, 0])).permute([2, 0, 1])
            if self.cfg.TM.use and self.training:
                x = time_mask(x, self.cfg.TM.t, self.cfg.TM.m, self.cfg.TM.p, replace_with_zero=True)
            frames.append(x.squeeze(1))
        f2 = torch.cat(frames, 0)
        fpe = [_frame_pos(self.frame_pe, s.unsqueeze(1)) for s in seq_list]
        fpos = None if fpe[0] is None else torch.cat([p.squeeze(1) for p in fpe], 0)
        # one shared gradient buffer for the query table's readers (fxf.PosGradSink: no pairwise adds)
        apos = fxf.pos_sink(self.action_query.squeeze(1).repeat(nvid, 1))
        a2 = torch.zeros_like(apos)
        for blk in self.block_list:
            f2, a2 = blk.forward_batch(f2, a2, fpos, apos, vb)
        self._vb = vb

        def restore(v):
            for blk in self.block_list:
                _set_side(blk, blk._vrec[v])
        return restore

    def _forward_lockstep(self, seq_list, label_list, compute_loss):
        """``forward`` for a batch ``_lockstep_ok`` accepts.  A batch in which a video's match exceeds
        FX_LOSS_MAXK runs its losses and predictions per video on the lockstep outputs, as
        blocks._forward_videos does on TableTooLarge."""
        nvid = len(seq_list)
        early = None
        if compute_loss:
            early = vn_vloss.BatchMatch(self, [blocks._label_to_host(l_) for l_ in label_list])
        restore = self._forward_batch(seq_list, early)
        restore(nvid - 1)       # side-channel attributes: the last video's views, as in the reference
        self.video_segments = [[blk._bt["S"][v] for blk in self.block_list] for v in range(nvid)]
        try:
            return vn_vloss.run_batch(self, self._vb, compute_loss, early)
        except vloss.TableTooLarge:
            pass
        save_list, final_loss, preds = [], [], []
        for v in range(nvid):
            restore(v)
            preds.append(self.block_list[-1].eval(None))
            save_list.append({})
            if compute_loss:
                final_loss.append(self._loss_one_video(label_list[v]))
        return self._read_back(save_list, preds, final_loss, compute_loss)

    def forward(self, seq_list, label_list, compute_loss=False):
        if LOCKSTEP and _lockstep_ok(self, seq_list):
            return self._forward_lockstep(seq_list, label_list, compute_loss)
        save_list, final_loss, preds = [], [], []
        for seq, label in zip(seq_list, label_list):
            trans = torch_class_label_to_segment_label(label)[0] if self.cfg.FACT.trans else None
            self._forward_one_video(seq.unsqueeze(1), trans)
            preds.append(self.block_list[-1].eval(trans))
            save_data = {}
            save_list.append(save_data)
            if compute_loss:
                final_loss.append(self._loss_one_video(label))
        return self._read_back(save_list, preds, final_loss, compute_loss)

    @staticmethod
    def _read_back(save_list, preds, final_loss, compute_loss):
        # one read-back for every video's predictions, loss floats and the kernels' status word
        dev = preds[0].device
        parts = [p.reshape(-1).to(torch.float64) for p in preds]
        parts += [lo.detach().reshape(1).to(torch.float64) for lo in final_loss]
        if dev.type == "cuda":
            parts.append(fxf.device_status(dev)[:1].to(torch.float64))
        host = torch.cat(parts).cpu().numpy()
        if dev.type == "cuda":
            fxf.status_raise(int(host[-1]), dev)
        off = 0
        for save_data, p in zip(save_list, preds):
            save_data["pred"] = host[off:off + p.numel()].astype("int64")
            off += p.numel()
        if compute_loss:
            for save_data, lo in zip(save_list, host[off:off + len(final_loss)]):
                save_data["loss"] = {"loss": float(lo)}
            return sum(final_loss) / len(final_loss), save_list
        return save_list

    def save_model(self, fname):
        torch.save(self.state_dict(), fname)


class Block(nn.Module):
    """blocks_SepVerbNoun.py:177-355."""

    # side-channel tables nothing on the fused path reads: built on first read
    frame_logp = _lazy_attr("frame_logp")
    seg_logp = _lazy_attr("seg_logp")
    # frame-level gathers of the segment attention rows (a2f_seg_attn / f2a_seg_attn, (1, S, Q))
    a2f_attn = _lazy_attr("a2f_attn")
    f2a_attn = _lazy_attr("f2a_attn")

    def __repr__(self):
        return (f"{type(self).__name__}(\n  f:{self.frame_branch},\n  a:{self.action_branch},\n"
                f"  a2f:{getattr(self, 'a2f_layer', None)},\n  f2a:{getattr(self, 'f2a_layer', None)}\n)")

    def combine_verb_noun_to_action(self, clogit, action=False, apply_log=True):
        """Action log-probabilities (T, 1, A (+ 1 null column)) of verb/noun class logits (T, 1, n1 + n2)."""
        if not apply_log:
            raise NotImplementedError("combine_verb_noun_to_action: only the log form is used (and built)")
        return fxf.verb_noun_logp(clogit, self.vnmap, action=action).unsqueeze(1)

    def process_feature(self, feature, nclass1, nclass2):
        out, clogit = fxf.process_feature(feature, nclass1 + nclass2, class_sep=nclass1)
        return out.unsqueeze(1), clogit.unsqueeze(1)

    def create_fbranch(self, cfg, in_dim=None, f_inmap=False):
        if in_dim is None:
            in_dim = cfg.f_dim
        if cfg.f == "m":
            return basic.MSTCN(in_dim, cfg.f_dim, cfg.hid_dim, cfg.f_layers, dropout=cfg.dropout, ln=cfg.f_ln,
                               ngroup=cfg.f_ngp, in_map=f_inmap)
        if cfg.f == "m2":
            return basic.MSTCN2(in_dim, cfg.f_dim, cfg.hid_dim, cfg.f_layers, dropout=cfg.dropout, ln=cfg.f_ln,
                                ngroup=cfg.f_ngp, in_map=f_inmap)
        raise ValueError(f"frame branch type {cfg.f!r} (the reference builds only 'm' / 'm2')")

    def create_abranch(self, cfg):
        if cfg.a == "sa":
            layer = basic.SALayer(cfg.a_dim, cfg.a_nhead, dim_feedforward=cfg.a_ffdim, dropout=cfg.dropout,
                                  attn_dropout=cfg.dropout)
            return basic.SADecoder(cfg.a_dim, cfg.a_dim, cfg.hid_dim, layer, cfg.a_layers, in_map=False)
        if cfg.a == "sca":
            layer = basic.SCALayer(cfg.a_dim, cfg.hid_dim, cfg.a_nhead, cfg.a_ffdim, dropout=cfg.dropout,
                                   attn_dropout=cfg.dropout)
            norm = torch.nn.LayerNorm(cfg.a_dim)
            return basic.SCADecoder(cfg.a_dim, cfg.a_dim, cfg.hid_dim, layer, cfg.a_layers, norm=norm, in_map=False)
        if cfg.a in ("gru", "gru_om"):
            assert self.cfg.FACT.trans
            return basic.ActionUpdate_GRU(cfg.a_dim, cfg.a_dim, cfg.hid_dim, cfg.a_layers, dropout=cfg.dropout,
                                          out_map=(cfg.a == "gru_om"))
        raise ValueError(cfg.a)

    def create_cross_attention(self, cfg, outdim, kq_pos=True):
        return basic.X2Y_map(cfg.hid_dim, cfg.hid_dim, outdim, head_dim=cfg.hid_dim, dropout=cfg.dropout,
                             kq_pos=kq_pos)

    def action_token_loss(self, criterion: MatchCriterion, match, action_logp):
        """blocks_SepVerbNoun.py:271-283: weighted one-hot NLL of the token log-probabilities, mean
        over tokens (unmatched tokens target the null column)."""
        logp = action_logp.squeeze(1)
        aind, sind = criterion._dev_match(match, logp.device)
        A, C = logp.shape[0], logp.shape[-1]
        clabel = torch.zeros(A, C, dtype=torch.long, device=logp.device)
        clabel[:, -1] = 1
        clabel[aind] = 0
        clabel[aind, criterion.transcript[sind]] = 1
        return ((-logp * clabel) * criterion.cweight).sum(-1).mean()

    def temporal_downsample(self, frame_feature):
        n1, n2 = self.nclass1, self.nclass2
        f2 = fxf._2d(frame_feature)
        tdu = basic.TemporalDownsampleUpsample.from_vn_probs(f2, f2.shape[1] - n1 - n2, n1, n2, self.vnmap)
        seg = tdu.feature_frame2seg(frame_feature)
        seg = fxf.gru(self.seg_update, seg, relu=True)            # relu(seg_update(seg))
        seg = fxf.linear(seg, self.seg_combine.weight, self.seg_combine.bias).unsqueeze(1)
        seg, seg_clogit = self.process_feature(seg, n1, n2)
        return tdu, seg, seg_clogit

    def temporal_upsample(self, tdu, seg_feature, frame_feature):
        lin = self.sf_merge[0]
        y = fxf.SegMergeFn.apply(fxf._2d(seg_feature), fxf._2d(frame_feature), tdu.seg_id32, tdu.start32, tdu.end32,
                                 lin.weight, lin.bias)
        return y.unsqueeze(1)

    def _downsample_batch(self, f2, fpos, vb):
        """``temporal_downsample`` over the stacked videos: one segmentation launch + ONE host read of every
        video's S (the first block: the loss phase's label-only host work runs while the host waits),
        segment means on the global tables, the BiGRU over the ragged segment rows.  Returns the segment
        record and (seg feature, seg class logits, seg positions)."""
        n1, n2 = self.nclass1, self.nclass2
        hook, vb.while_waiting = vb.while_waiting, None
        S, local, (gid, gst, gen) = fxf.segments_from_vn_probs_batched(f2, f2.shape[1] - n1 - n2, n1, n2, self.vnmap,
                                                                        vb.f_off, hook)
        s_off = [0]
        for n_ in S:
            s_off.append(s_off[-1] + n_)
        seg = fxf.SegMeanFn.apply(f2, gid, gst, gen)
        seg = fxf.gru(self.seg_update, seg, seq_off=s_off, relu=True)     # relu(seg_update(seg))
        seg = fxf.linear(seg, self.seg_combine.weight, self.seg_combine.bias)
        seg_out, seg_cl = fxf.process_feature(seg, n1 + n2, class_sep=n1)
        seg_pos = None
        if fpos is not None:
            seg_pos = fpos[torch.div(gst + gen, 2, rounding_mode="floor").to(torch.int64)]
        return dict(S=S, s_off=s_off, local=local, glob=(gid, gst, gen)), seg_out, seg_cl, seg_pos

    def _save_batch(self, vb, sg, f_cl, seg_cl, a_cl, attn=None):
        """Per-video side channels of the stacked outputs as views through one split node per tensor
        (``_vrec``: what ``_save_logp`` / ``_save_attn`` set for one video), and the stacked tensors the
        loss phase reads (``_bt``)."""
        Q, S, nvid = vb.Q, sg["S"], vb.nvid
        fc, ac, sc = vb.frames(f_cl), vb.tokens(a_cl), torch.split(seg_cl, S)
        alp = vb.tokens(fxf.verb_noun_logp(a_cl, self.vnmap, action=True))
        tdus = [basic.TemporalDownsampleUpsample(*sg["local"][v]) for v in range(nvid)]
        bt = dict(f_cl=f_cl, seg_cl=seg_cl, a_cl=a_cl, S=S, s_off=sg["s_off"], local=sg["local"])
        if attn is not None:
            f2a_lg, f2a_at, a2f_lg, a2f_at = attn
            qs = [Q * n_ for n_ in S]
            fat, aat, flg, alg = (torch.split(t, qs) for t in (f2a_at, a2f_at, f2a_lg, a2f_lg))
            bt.update(f2a_lg=f2a_lg, a2f_lg=a2f_lg, a2f_at=a2f_at)
        recs = []
        for v in range(nvid):
            fcv, scv, tdu = fc[v].unsqueeze(1), sc[v].unsqueeze(1), tdus[v]
            rec = dict(_fused=True, _clogits=(fcv, scv, ac[v].unsqueeze(1)), tdu=tdu,
                       seg_logp=_Lazy(lambda c=scv: self.combine_verb_noun_to_action(c)),
                       frame_logp=_Lazy(lambda c=fcv: self.combine_verb_noun_to_action(c)),
                       action_logp=alp[v].unsqueeze(1))
            if attn is None:
                rec.update(f2a_seg_attn=None, a2f_seg_attn=None, f2a_attn=None, a2f_attn=None)
            else:
                Sv = S[v]
                f2a_seg, a2f_seg = fat[v].view(1, Q, Sv).transpose(2, 1), aat[v].view(1, Sv, Q)
                rec.update(f2a_seg_attn=f2a_seg, a2f_seg_attn=a2f_seg,
                           f2a_attn=_Lazy(lambda t=tdu, a=f2a_seg: t.attn_seg2frame(a).transpose(2, 1)),
                           a2f_attn=_Lazy(lambda t=tdu, a=a2f_seg: t.attn_seg2frame(a)),
                           f2a_attn_logit=flg[v].view(1, Q, Sv), a2f_attn_logit=alg[v].view(1, Sv, Q))
            recs.append(rec)
        self.__dict__["_vrec"] = recs     # (plain attributes: no nn.Module.__setattr__ walk)
        self.__dict__["_bt"] = bt

    def _save_logp(self, frame_clogit, seg_clogit, action_clogit, tdu):
        self._fused = FUSED_LOSS and frame_clogit.is_cuda
        self._clogits = (frame_clogit, seg_clogit, action_clogit) if self._fused else None
        if self._fused:
            self.seg_logp = _Lazy(lambda c=seg_clogit: self.combine_verb_noun_to_action(c))
            self.frame_logp = _Lazy(lambda c=frame_clogit: self.combine_verb_noun_to_action(c))
        else:
            self.seg_logp = self.combine_verb_noun_to_action(seg_clogit)
            self.frame_logp = self.combine_verb_noun_to_action(frame_clogit)
        self.action_logp = self.combine_verb_noun_to_action(action_clogit, action=True)
        self.tdu = tdu

    def _save_attn(self, tdu, f2a_seg, a2f_seg):
        """The cross-attention side channels: the (1, S, Q) segment rows as they are, and the reference's
        frame-level ``f2a_attn`` (1, Q, T) / ``a2f_attn`` (1, T, Q) gathered on first read."""
        self.f2a_seg_attn, self.a2f_seg_attn = f2a_seg, a2f_seg
        if tdu is None:
            self.f2a_attn = self.a2f_attn = None
            return
        self.f2a_attn = _Lazy(lambda: tdu.attn_seg2frame(f2a_seg).transpose(2, 1))
        self.a2f_attn = _Lazy(lambda: tdu.attn_seg2frame(a2f_seg))

    def _token_loss(self, criterion: MatchCriterion, match):
        if self._fused:
            return criterion.vn_token_terms(match, self._clogits[2], self.vnmap)
        return self.action_token_loss(criterion, match, self.action_logp)

    def _frame_seg_loss(self, criterion):
        if self._fused:
            # (frame_loss / 2 + frame_loss_tdu / 2) / 2 + sw * smooth_loss, two launch pairs
            fl = criterion.vn_frame_terms(self._clogits[0], self.vnmap, ce_coef=0.25, sm_coef=self.cfg.Loss.sw)
            return fl + criterion.vn_seg_terms(self._clogits[1], self.vnmap, self.tdu, ce_coef=0.25)
        frame_loss = criterion.frame_loss(self.frame_logp.squeeze(1), is_logit=False) / 2
        seg_loss = criterion.frame_loss_tdu(self.seg_logp, self.tdu, is_logit=False) / 2
        sl = loss.smooth_loss(torch.transpose(self.frame_logp, 0, 1), is_logit=False)
        return (frame_loss + seg_loss) / 2 + self.cfg.Loss.sw * sl

    @staticmethod
    def _eval(action_logp, a2f_attn, frame_logp, weight):
        """blocks_SepVerbNoun.py:323-342 without a host sync: null tokens are masked to -inf before
        the argmax over tokens (first maximum, as the reference's argmax over the non-null subset);
        with no non-null token the frame branch decides alone."""
        fprob = torch.exp(frame_logp.squeeze(1))
        alp = action_logp.squeeze(1)
        a2f = a2f_attn.squeeze(0)
        is_tok = alp.argmax(1) != alp.shape[-1] - 1
        masked = torch.where(is_tok[None, :], a2f, torch.full((), float("-inf"), device=a2f.device, dtype=a2f.dtype))
        qtk_prob = torch.exp(alp[:, :-1])
        qtk_prob = qtk_prob / qtk_prob.sum(-1, keepdim=True)
        mixed = ((1 - weight) * qtk_prob[masked.argmax(-1)] + weight * fprob).argmax(1)
        return torch.where(is_tok.any(), mixed, fprob.argmax(1))

    @staticmethod
    def _eval_w_transcript(transcript, a2f_attn):
        n = len(transcript)
        return transcript[a2f_attn[0, :, :n].argmax(1)]

    def eval(self, transcript=None):
        if not self.cfg.FACT.trans:
            if self._fused and self.a2f_seg_attn is not None:
                return fxf.vn_eval_pred(self._clogits[2], self._clogits[0], self.a2f_seg_attn, self.vnmap,
                                        self.cfg.FACT.mwt, seg_id=self.tdu.seg_id32)
            if self._fused:
                return fxf.vn_eval_pred(self._clogits[2], self._clogits[0], self.a2f_attn, self.vnmap,
                                        self.cfg.FACT.mwt)
            return self._eval(self.action_logp, self.a2f_attn, self.frame_logp, self.cfg.FACT.mwt)
        return self._eval_w_transcript(transcript, self.a2f_attn)


class InputBlockTDU(Block):
    """blocks_SepVerbNoun.py:358-413."""

    def __init__(self, cfg, in_dim, nclass1, nclass2, vnmap):
        super().__init__()
        self.cfg = cfg
        self.nclass1 = nclass1
        self.nclass2 = nclass2
        self.vnmap = vnmap
        bcfg = cfg.Bi
        self.frame_branch = self.create_fbranch(bcfg, in_dim, f_inmap=True)
        self.action_branch = self.create_abranch(bcfg)
        self.seg_update = nn.GRU(bcfg.hid_dim, bcfg.hid_dim // 2, 2, bidirectional=True)
        self.seg_combine = nn.Linear(bcfg.hid_dim, bcfg.hid_dim)

    def forward(self, frame_feature, action_feature, frame_pos, action_pos):
        frame_feature = self.frame_branch(frame_feature)
        frame_feature, frame_clogit = self.process_feature(frame_feature, self.nclass1, self.nclass2)
        tdu, seg_feature, seg_clogit = self.temporal_downsample(frame_feature)
        seg_pos = None if frame_pos is None else frame_pos[tdu.centers()]
        action_feature = self.action_branch(action_feature, seg_feature, pos=seg_pos, query_pos=action_pos)
        action_feature, action_clogit = self.process_feature(action_feature, self.nclass1 + 1, self.nclass2 + 1)
        self._save_logp(frame_clogit, seg_clogit, action_clogit, tdu)
        self._save_attn(None, None, None)
        return frame_feature, action_feature

    def forward_batch(self, f2, a2, fpos, apos, vb):
        """``forward`` over vb.nvid stacked videos (frames (sum T, C), tokens (nvid * Q, A)): the SCA decoder
        reads each video's segment rows through the ragged memory offsets."""
        n1, n2 = self.nclass1, self.nclass2
        f = _frame_branch_batch(self.frame_branch, f2, vb)
        f_out, f_cl = fxf.process_feature(f, n1 + n2, class_sep=n1)
        sg, seg_out, seg_cl, seg_pos = self._downsample_batch(f_out, fpos, vb)
        a = fxf.decoder(self.action_branch, a2, seg_out, pos=seg_pos, query_pos=apos, nvid=vb.nvid,
                        mem_off=sg["s_off"])
        a_out, a_cl = fxf.process_feature(a, n1 + n2 + 2, class_sep=n1 + 1)
        self._save_batch(vb, sg, f_cl, seg_cl, a_cl)
        return f_out, a_out

    def compute_loss(self, criterion: MatchCriterion, match=None):
        atk_loss = self._token_loss(criterion, match) / 2
        return self._frame_seg_loss(criterion) + atk_loss


class UpdateBlockTDU(Block):
    """blocks_SepVerbNoun.py:415-496: segment-level update with temporal down/up-sampling."""

    def __init__(self, cfg, nclass1, nclass2, vnmap):
        super().__init__()
        self.cfg = cfg
        self.nclass1 = nclass1
        self.nclass2 = nclass2
        self.vnmap = vnmap
        bcfg = cfg.BU
        self.frame_branch = self.create_fbranch(bcfg)
        self.seg_update = nn.GRU(bcfg.hid_dim, bcfg.hid_dim // 2, bcfg.s_layers, bidirectional=True)
        self.seg_combine = nn.Linear(bcfg.hid_dim, bcfg.hid_dim)
        self.f2a_layer = self.create_cross_attention(bcfg, bcfg.a_dim)
        self.action_branch = self.create_abranch(bcfg)
        self.a2f_layer = self.create_cross_attention(bcfg, bcfg.f_dim)
        self.sf_merge = nn.Sequential(nn.Linear(bcfg.hid_dim + bcfg.f_dim, bcfg.f_dim), nn.ReLU())

    def forward(self, frame_feature, action_feature, frame_pos, action_pos):
        tdu, seg_feature, seg_clogit = self.temporal_downsample(frame_feature)
        seg_pos = None if frame_pos is None else frame_pos[tdu.centers()]
        action_feature = self.f2a_layer(seg_feature, action_feature, X_pos=seg_pos, Y_pos=action_pos)
        action_feature = self.action_branch(action_feature, action_pos)
        action_feature, action_clogit = self.process_feature(action_feature, self.nclass1 + 1, self.nclass2 + 1)
        seg_feature = self.a2f_layer(action_feature, seg_feature, X_pos=action_pos, Y_pos=seg_pos)
        frame_feature = self.temporal_upsample(tdu, seg_feature, frame_feature)
        frame_feature = self.frame_branch(frame_feature)
        frame_feature, frame_clogit = self.process_feature(frame_feature, self.nclass1, self.nclass2)
        self._save_logp(frame_clogit, seg_clogit, action_clogit, tdu)
        self.f2a_attn_logit = self.f2a_layer.attn_logit.squeeze(0).unsqueeze(0)
        self.a2f_attn_logit = self.a2f_layer.attn_logit.squeeze(0).unsqueeze(0)
        self._save_attn(tdu, self.f2a_layer.attn[0].transpose(2, 1), self.a2f_layer.attn[0])
        return frame_feature, action_feature

    def forward_batch(self, f2, a2, fpos, apos, vb):
        n1, n2 = self.nclass1, self.nclass2
        sg, seg_out, seg_cl, seg_pos = self._downsample_batch(f2, fpos, vb)
        s_off = sg["s_off"]
        f2a, a2f = self.f2a_layer, self.a2f_layer
        a, f2a_lg, f2a_at = fxf.x2y(f2a, seg_out, a2, seg_pos if f2a.kq_pos else None, apos if f2a.kq_pos else None,
                                    rows=(s_off, vb.a_off))
        a = fxf.decoder(self.action_branch, a, None, query_pos=apos, nvid=vb.nvid)
        a_out, a_cl = fxf.process_feature(a, n1 + n2 + 2, class_sep=n1 + 1)
        sgf, a2f_lg, a2f_at = fxf.x2y(a2f, a_out, seg_out, apos if a2f.kq_pos else None,
                                      seg_pos if a2f.kq_pos else None, rows=(vb.a_off, s_off))
        if vb.on_a2f is not None and vb.last is self:
            # the loss phase's matching starts here (vn_vloss.BatchMatch): its cost launch and read-back
            # queue ahead of sf_merge and the frame branch, the host matching overlaps them
            vb.on_a2f(vb, a_cl, a2f_at, (s_off, sg["local"]))
        gid, gst, gen = sg["glob"]
        lin = self.sf_merge[0]
        f = fxf.SegMergeFn.apply(sgf, f2, gid, gst, gen, lin.weight, lin.bias)
        f = _frame_branch_batch(self.frame_branch, f, vb)
        f_out, f_cl = fxf.process_feature(f, n1 + n2, class_sep=n1)
        self._save_batch(vb, sg, f_cl, seg_cl, a_cl, (f2a_lg, f2a_at, a2f_lg, a2f_at))
        return f_out, a_out

    def compute_loss(self, criterion: MatchCriterion, match=None):
        atk_loss = self._token_loss(criterion, match) / 2
        f2a_loss = criterion.cross_attn_loss_tdu(match, torch.transpose(self.f2a_attn_logit, 1, 2), self.tdu, dim=1)
        a2f_loss = criterion.cross_attn_loss_tdu(match, self.a2f_attn_logit, self.tdu, dim=2)
        return self._frame_seg_loss(criterion) + atk_loss + f2a_loss + a2f_loss
