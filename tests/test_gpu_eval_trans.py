"""fx_eval_pred_trans (csrc/vloss.hip) against the float64 ``Block._eval_w_transcript`` (GPU).

The kernel's blended probability carries a few fp32 roundings per term (two softmaxes, one blend: relative
error of a few 1e-7, measured 2-4e-7 on the reference's own float32 run).  Inputs are
drawn by seeded rejection until every frame's float64 relative margin between the best position and the best
position of ANOTHER class is >= 1e-4 (positions of one class give the same prediction), 100x that error, so
every frame of every case is compared and none is skipped.
"""
import ctypes

import numpy as np
import pytest
import torch

from factmx import native as nx
from factmx.models.blocks import Block
from factmx.models.termtable import _Pack

pytestmark = pytest.mark.gpu
DEV = "cuda"
MIN_MARGIN = 1e-4


def _reference(v, mwt):
    """(pred, class-level relative margin per frame) of one video in float64."""
    attn = v["attn"].double()
    a2f = (attn if v["seg_id"] is None else attn[v["seg_id"].long()])[None]          # (1, T, Q)
    tr = torch.from_numpy(v["gl"].astype(np.int64))
    pred = Block._eval_w_transcript(tr, a2f, v["flogit"].double()[:, None], mwt)
    fprob = torch.softmax(v["flogit"].double(), -1)[:, tr]
    p = (1 - mwt) * torch.softmax(a2f[0, :, :len(tr)], -1) + mwt * fprob
    top, arg = p.max(1)
    other = torch.where(tr[None, :] != tr[arg][:, None], p, torch.zeros_like(p)).max(1).values
    return pred.numpy(), ((top - other) / top).numpy()


def _video(T, N, C, Q, S, seed, mwt, tie=None, distinct=False):
    """A video (float32 inputs) whose every frame has a class-level margin >= MIN_MARGIN in float64.
    ``S``: None frame-level attention, else the number of segment rows.  ``tie`` = (frame, n1, n2): that
    frame gets equal logits for the classes of positions n1 < n2 and equal, dominant attention columns.
    ``distinct``: a transcript without repeated classes (N <= C), so that the class-level margin IS the margin
    between any two positions and the kernel's choice of position is compared with the reference's."""
    for k in range(400):
        g = torch.Generator().manual_seed(1000 * seed + k)
        gl = torch.randint(0, C, (N,), generator=g).numpy().astype(np.int32)
        if distinct:
            gl = torch.randperm(C, generator=g).numpy()[:N].astype(np.int32)
        elif N >= 3:
            gl[2] = gl[0]                                   # a transcript with duplicate classes
        if tie is not None:
            gl[tie[1]], gl[tie[2]] = 0, C - 1
        flogit = (2.0 * torch.randn(T, C, generator=g)).float()
        rows = T if S is None else S
        attn = torch.softmax(3.0 * torch.randn(rows, Q, generator=g), -1).float()
        seg_id = None
        if S is not None:
            cuts = np.sort(torch.randperm(T - 1, generator=g).numpy()[:S - 1] + 1) if S > 1 else np.zeros(0, int)
            seg_id = torch.from_numpy(np.searchsorted(cuts, np.arange(T), side="right").astype(np.int32))
        if tie is not None:
            t0, n1, n2 = tie
            r0 = t0 if seg_id is None else int(seg_id[t0])
            attn[r0, n1] = attn[r0, n2] = attn[r0].max() + 0.25
            flogit[t0, 0] = flogit[t0, C - 1] = flogit[t0].max() + 1.0
        v = dict(T=T, N=N, C=C, Q=Q, gl=gl, flogit=flogit, attn=attn, seg_id=seg_id)
        pred, margin = _reference(v, mwt)
        if tie is not None:
            margin = np.delete(margin, tie[0])
        if (margin >= MIN_MARGIN).all():
            v["pred"] = pred
            return v
    raise AssertionError("no inputs with the required margins in 400 draws")


def _launch(videos, mwt, edit=None, lead=3):
    """fx_eval_pred_trans over ``videos``; returns (status, pred buffer on the host, per-video offsets)."""
    lib = nx.load()
    pk = _Pack()
    off, va = pk.structs(nx.VideoAttn, len(videos))
    base = pk.alloc(DEV)
    keep, offs, n = [], [], lead
    for v, a in zip(videos, va):
        fl, at = v["flogit"].to(DEV), v["attn"].to(DEV)
        gl = torch.from_numpy(v["gl"]).to(DEV)
        sid = None if v["seg_id"] is None else v["seg_id"].to(DEV)
        keep += [fl, at, gl, sid]
        a.Q, a.C1, a.T, a.G = v["Q"], v["C"] + 1, v["T"], v["N"]
        a.attn, a.lda = at.data_ptr(), v["Q"]
        a.seg_id = None if sid is None else sid.data_ptr()
        a.flogit, a.ldf = fl.data_ptr(), v["C"]
        a.gl, a.pred_off = gl.data_ptr(), n
        offs.append(n)
        n += v["T"]
    if edit is not None:
        edit(va)
    pk.send()
    pred = torch.full((n + 2,), -1, dtype=torch.int32, device=DEV)
    st = lib.fx_eval_pred_trans(ctypes.addressof(va), base + off, len(videos), float(mwt), pred.data_ptr(), nx.stream())
    torch.cuda.synchronize()
    return st, pred.cpu().numpy(), offs


def _check(videos, mwt):
    st, pred, offs = _launch(videos, mwt)
    assert st == 0, nx.load().fx_last_error()
    seen = np.zeros(len(pred), dtype=bool)
    for v, o in zip(videos, offs):
        np.testing.assert_array_equal(pred[o:o + v["T"]], v["pred"])
        seen[o:o + v["T"]] = True
    assert (pred[~seen] == -1).all(), "frames outside the videos' pred_off ranges were written"


# (T, N, C, Q, S)
SHAPES = {
    "T=1": (1, 1, 2, 1, None),
    "frame-level": (33, 2, 5, 5, None),
    "segment-level S=1": (211, 5, 12, 8, 1),
    "segment-level S=T": (211, 5, 12, 8, 211),
    "segment-level": (211, 5, 12, 8, 17),
    "70 tokens": (64, 70, 12, 70, None),
    "two workgroups": (300, 5, 12, 5, None),
}


@pytest.mark.parametrize("mwt", [0.0, 0.1, 1.0])
@pytest.mark.parametrize("nvid", [1, 3])
@pytest.mark.parametrize("name", list(SHAPES))
def test_prediction_matches_float64(name, nvid, mwt):
    T, N, C, Q, S = SHAPES[name]
    videos = [_video(T, N, C, Q, S, seed=1, mwt=mwt)]
    if nvid == 3:       # ragged: other lengths, another transcript length, frame- and segment-level mixed
        videos.append(_video(T + 5, max(N - 1, 1), C, Q, None, seed=2, mwt=mwt))
        videos.append(_video(max(T // 2, 1), N, C, Q, None if S is None else max(1, min(S, T // 2) // 2), seed=3,
                             mwt=mwt))
    _check(videos, mwt)


@pytest.mark.parametrize("mwt", [0.0, 0.1, 1.0])
@pytest.mark.parametrize("T,N,C,Q,S", [(211, 5, 12, 8, 17), (33, 12, 12, 12, None), (300, 7, 9, 7, 300)])
def test_the_chosen_position_matches_float64(T, N, C, Q, S, mwt):
    """Transcripts without repeated classes: every position has its own class, so every frame's margin between
    ANY two positions is >= 1e-4 and the predicted class identifies the position the kernel chose."""
    v = _video(T, N, C, Q, S, seed=11, mwt=mwt, distinct=True)
    assert len(set(v["gl"].tolist())) == N
    _check([v], mwt)


@pytest.mark.parametrize("S", [None, 9])
def test_an_exact_tie_takes_the_first_position(S):
    v = _video(33, 4, 5, 6, S, seed=5, mwt=0.1, tie=(7, 1, 3))
    assert v["gl"][1] == 0 and v["gl"][3] == 4 and v["pred"][7] == 0      # float64 torch: the first maximum
    _check([v], 0.1)


def test_bad_arguments_are_refused_before_any_launch():
    lib = nx.load()
    v = _video(33, 2, 5, 5, None, seed=1, mwt=0.1)

    def setter(**kw):
        def edit(va):
            for k, val in kw.items():
                setattr(va[0], k, val)
        return edit
    for bad, text in ((dict(G=6), b"G > Q"), (dict(gl=None), b"without a transcript"), (dict(C1=1), b"without logits"),
                      (dict(G=0), b"empty transcript"), (dict(flogit=None), b"without logits")):
        st, pred, _ = _launch([v], 0.1, edit=setter(**bad))
        assert st != 0 and text in lib.fx_last_error(), bad
        assert (pred == -1).all(), "a refused call must not launch"
