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

This file holds what is particular to the verb/noun heads: the mapping, ``VerbNounHeads`` (the class
columns and the segmentation, as blocks.ClassHeads), ``Block`` (action log-probabilities, loss helpers,
prediction, the lazy ``frame_logp`` / ``seg_logp`` and the side channels ``_save_logp`` / ``_save_attn`` /
``_save_batch``), the input block, the transcript embedding and the ``forward`` drivers with their read-back.
The branch constructors (blocks.Block), the segment-level flow of both blocks for one video and for stacked
videos (blocks._TDU), the per-video views (blocks._save_views) and the model's walk through the blocks
(blocks._FACTBase._run_blocks / _forward_batch) are shared with models.blocks.
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
from .basic import torch_class_label_to_segment_label
from .blocks import _frame_branch_batch, _Lazy, _lazy_attr
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


class FACT(blocks._FACTBase):
    """blocks_SepVerbNoun.py:14-142.  The blocks run through the base's ``_run_blocks`` (one video) and
    ``_forward_batch`` (lockstep)."""

    dp_marks = False              # no factmx.dp marks on this model's block inputs
    # the last block starts the matching (vn_vloss.BatchMatch) before sf_merge: its cost launch and read-back
    # queue ahead of sf_merge and the frame branch, the host matching overlaps them
    match_before_merge = True

    def __init__(self, cfg, in_dim, n_classes1=98, n_classes2=301):
        super().__init__()
        self.vnmap = init_VIDS_NIDS()
        # the reference asserts this on every forward (blocks_SepVerbNoun.py:198-207)
        if (n_classes1, n_classes2) != (self.vnmap.num_verbs, self.vnmap.num_nouns):
            raise ValueError(f"{n_classes1} verb / {n_classes2} noun classes, but the installed mapping has "
                             f"{self.vnmap.num_verbs} / {self.vnmap.num_nouns}")
        self.num_classes1 = n_classes1   # verbs
        self.num_classes2 = n_classes2   # nouns
        self._init_common(cfg)
        base_cfg = cfg.Bi
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

    def _create_embed(self, a_dim):
        self.verb_embed = nn.Embedding(self.num_classes1, a_dim // 2)
        self.noun_embed = nn.Embedding(self.num_classes2, a_dim // 2)

    def _transcript_tokens(self, transcript):
        vtranscript, ntranscript = self.vnmap.verb_noun_of(transcript)
        action_pe = self.action_pe(transcript)
        vfeature = self.verb_embed(vtranscript).unsqueeze(1)
        nfeature = self.noun_embed(ntranscript).unsqueeze(1)
        return torch.cat([vfeature, nfeature], dim=-1) + action_pe, torch.zeros_like(action_pe)

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


class VerbNounHeads:
    """blocks.ClassHeads for n1 verb + n2 noun class columns, each group with its own softmax (token rows:
    one null column more per group); frames are segmented by the argmax over the mapped actions."""

    def __init__(self, nclass1, nclass2, vnmap):
        self.n1, self.n2, self.vnmap = nclass1, nclass2, vnmap

    def split(self, x):
        return fxf.process_feature(x, self.n1 + self.n2, class_sep=self.n1)

    def split_tokens(self, x):
        return fxf.process_feature(x, self.n1 + self.n2 + 2, class_sep=self.n1 + 1)

    def segment(self, f2):
        n1, n2 = self.n1, self.n2
        return basic.TemporalDownsampleUpsample.from_vn_probs(f2, f2.shape[1] - n1 - n2, n1, n2, self.vnmap)

    def segment_batch(self, f2, f_off, hook):
        n1, n2 = self.n1, self.n2
        return fxf.segments_from_vn_probs_batched(f2, f2.shape[1] - n1 - n2, n1, n2, self.vnmap, f_off, hook)


class Block(blocks.Block):
    """blocks_SepVerbNoun.py:177-355: the verb/noun heads on the shared branches (``create_*``) and
    side-channel plumbing of blocks.Block.  ``a2f_attn`` / ``f2a_attn`` (lazy there too) are the frame-level
    gathers of the segment attention rows (``a2f_seg_attn`` / ``f2a_seg_attn``, (1, S, Q))."""

    # side-channel tables nothing on the fused path reads: built on first read
    frame_logp = _lazy_attr("frame_logp")
    seg_logp = _lazy_attr("seg_logp")

    def _init_heads(self, cfg, nclass1, nclass2, vnmap):
        self.cfg = cfg
        self.nclass1 = nclass1
        self.nclass2 = nclass2
        self.vnmap = vnmap
        self.heads = VerbNounHeads(nclass1, nclass2, vnmap)

    def combine_verb_noun_to_action(self, clogit, action=False, apply_log=True):
        """Action log-probabilities (T, 1, A (+ 1 null column)) of verb/noun class logits (T, 1, n1 + n2)."""
        if not apply_log:
            raise NotImplementedError("combine_verb_noun_to_action: only the log form is used (and built)")
        return fxf.verb_noun_logp(clogit, self.vnmap, action=action).unsqueeze(1)

    def process_feature(self, feature, nclass1, nclass2):
        out, clogit = fxf.process_feature(feature, nclass1 + nclass2, class_sep=nclass1)
        return out.unsqueeze(1), clogit.unsqueeze(1)

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

    def _save_batch(self, vb, sg, f_cl, seg_cl, a_cl, a_out=None, attn=None):
        """Per-video side channels of the stacked outputs (``_vrec``: what ``_save_logp`` / ``_save_attn``
        set for one video, on the views of blocks._save_views) and the stacked tensors the loss phase reads
        (``_bt``)."""
        views = blocks._save_views(self, vb, f_cl, a_cl, seg=(sg, seg_cl), attn=attn)
        alp = vb.tokens(fxf.verb_noun_logp(a_cl, self.vnmap, action=True))
        recs = []
        for v, w in enumerate(views):
            fcv, scv, tdu = w["frame_clogit"], w["seg_clogit"], w["tdu"]
            rec = dict(_fused=True, _clogits=(fcv, scv, w["action_clogit"]), tdu=tdu,
                       seg_logp=_Lazy(lambda c=scv: self.combine_verb_noun_to_action(c)),
                       frame_logp=_Lazy(lambda c=fcv: self.combine_verb_noun_to_action(c)),
                       action_logp=alp[v].unsqueeze(1))
            if attn is None:
                rec.update(f2a_seg_attn=None, a2f_seg_attn=None, f2a_attn=None, a2f_attn=None)
            else:
                f2a_seg, a2f_seg = w["f2a_attn"].transpose(2, 1), w["a2f_attn"]
                rec.update(f2a_seg_attn=f2a_seg, a2f_seg_attn=a2f_seg,
                           f2a_attn=_Lazy(lambda t=tdu, a=f2a_seg: t.attn_seg2frame(a).transpose(2, 1)),
                           a2f_attn=_Lazy(lambda t=tdu, a=a2f_seg: t.attn_seg2frame(a)),
                           f2a_attn_logit=w["f2a_attn_logit"], a2f_attn_logit=w["a2f_attn_logit"])
            recs.append(rec)
        self.__dict__["_vrec"] = recs     # (plain attributes: no nn.Module.__setattr__ walk)

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


class InputBlockTDU(blocks._TDU, Block):
    """blocks_SepVerbNoun.py:358-413: the input block reads the segments of its own frame branch (the
    down-sampling half of blocks._TDU)."""

    def __init__(self, cfg, in_dim, nclass1, nclass2, vnmap):
        super().__init__()
        self._init_heads(cfg, nclass1, nclass2, vnmap)
        bcfg = cfg.Bi
        self.frame_branch = self.create_fbranch(bcfg, in_dim, f_inmap=True)
        self.action_branch = self.create_abranch(bcfg)
        self._create_seg(bcfg, 2)

    def forward(self, frame_feature, action_feature, frame_pos, action_pos):
        frame_feature = self.frame_branch(frame_feature)
        frame_feature, frame_clogit = self._split(frame_feature)
        tdu, seg_feature, seg_clogit = self.temporal_downsample(frame_feature)
        seg_pos = None if frame_pos is None else frame_pos[tdu.centers()]
        action_feature = self.action_branch(action_feature, seg_feature, pos=seg_pos, query_pos=action_pos)
        action_feature, action_clogit = self._split(action_feature, tokens=True)
        self._save_logp(frame_clogit, seg_clogit, action_clogit, tdu)
        self._save_attn(None, None, None)
        return frame_feature, action_feature

    def forward_batch(self, f2, a2, fpos, apos, vb):
        """``forward`` over vb.nvid stacked videos (frames (sum T, C), tokens (nvid * Q, A)): the SCA decoder
        reads each video's segment rows through the ragged memory offsets."""
        f = _frame_branch_batch(self.frame_branch, f2, vb)
        f_out, f_cl = self.heads.split(f)
        sg, seg_out, seg_cl, seg_pos = self._downsample_batch(f_out, fpos, vb)
        a = fxf.decoder(self.action_branch, a2, seg_out, pos=seg_pos, query_pos=apos, nvid=vb.nvid,
                        mem_off=sg["s_off"])
        a_out, a_cl = self.heads.split_tokens(a)
        self._save_batch(vb, sg, f_cl, seg_cl, a_cl)
        return f_out, a_out

    def compute_loss(self, criterion: MatchCriterion, match=None):
        atk_loss = self._token_loss(criterion, match) / 2
        return self._frame_seg_loss(criterion) + atk_loss


class UpdateBlockTDU(blocks._TDU, Block):
    """blocks_SepVerbNoun.py:415-496: segment-level update with temporal down/up-sampling (the flow is
    blocks._TDU's ``forward`` / ``forward_batch``)."""

    def __init__(self, cfg, nclass1, nclass2, vnmap):
        super().__init__()
        self._init_heads(cfg, nclass1, nclass2, vnmap)
        self._create_update(cfg.BU)

    def _save(self, tdu, frame_clogit, seg_clogit, action_clogit, action_feature):
        self._save_logp(frame_clogit, seg_clogit, action_clogit, tdu)
        self.f2a_attn_logit = self.f2a_layer.attn_logit.squeeze(0).unsqueeze(0)
        self.a2f_attn_logit = self.a2f_layer.attn_logit.squeeze(0).unsqueeze(0)
        self._save_attn(tdu, self.f2a_layer.attn[0].transpose(2, 1), self.a2f_layer.attn[0])

    def compute_loss(self, criterion: MatchCriterion, match=None):
        atk_loss = self._token_loss(criterion, match) / 2
        f2a_loss = criterion.cross_attn_loss_tdu(match, torch.transpose(self.f2a_attn_logit, 1, 2), self.tdu, dim=1)
        a2f_loss = criterion.cross_attn_loss_tdu(match, self.a2f_attn_logit, self.tdu, dim=2)
        return self._frame_seg_loss(criterion) + atk_loss + f2a_loss + a2f_loss
