"""Ragged token rows in one decoder call / one transcript pass: the switch and the pass grouping, the row
layout of a batch with per-video token counts, and what the header and the binding declare (CPU)."""
import ctypes
import os
import re

import pytest
import torch

from factmx import native as nx
from factmx.models import blocks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_switch_is_off_by_default_and_groups_one_pass_when_on(monkeypatch):
    tp = blocks.transcript_passes
    ragged = [[2, 5, 9, 2, 5], [1, 2, 3, 4, 5], [7, 8, 9, 1]]
    assert blocks.TRANS_RAGGED is False
    assert tp(ragged) == [[0], [1], [2]] and tp(ragged[:2]) == [[0, 1]] and tp([[1, 2], [3]]) == [[0], [1]]
    monkeypatch.setattr(blocks, "TRANS_RAGGED", True)
    assert tp(ragged) == [[0, 1, 2]] and tp(ragged[:2]) == [[0, 1]] and tp([[1, 2], [3]]) == [[0, 1]]
    assert tp([[4]]) == [[0]] and tp([]) == []
    n = blocks.MAX_LOCKSTEP_VIDEOS
    assert tp([[1] * (1 + v % 3) for v in range(n)]) == [list(range(n))]
    # more videos than one pass takes still split
    assert tp([[1] * (1 + v % 3) for v in range(n + 1)]) == [[v] for v in range(n + 1)]


def test_video_batch_with_per_video_token_counts():
    vb = blocks._VideoBatch(3, [50, 7, 31], [5, 4, 1])
    assert vb.Qs == [5, 4, 1] and vb.a_off == [0, 5, 9, 10] and vb.tok_ragged and vb.tok_off == vb.a_off
    assert [vb.tk(v) for v in range(3)] == [slice(0, 5), slice(5, 9), slice(9, 10)]
    t = torch.arange(20.0).view(10, 2)
    parts = vb.tokens(t)
    assert [p.shape[0] for p in parts] == [5, 4, 1] and torch.equal(parts[1], t[5:9]) and torch.equal(parts[2], t[9:])
    assert vb.attn_off(vb.Ts) == [0, 250, 278, 309] and vb.attn_off([3, 2, 6]) == [0, 15, 23, 29]
    with pytest.raises(AttributeError):
        vb.Q                                         # not to be read when the counts differ
    # the int form (learned queries, the verb/noun model) and a list of equal counts: an even split
    for q in (8, [8, 8, 8]):
        vb = blocks._VideoBatch(3, [50, 7, 31], q)
        assert vb.Q == 8 and isinstance(vb.Q, int) and vb.Qs == [8, 8, 8] and vb.a_off == [0, 8, 16, 24]
        assert not vb.tok_ragged and vb.tok_off is None and vb.tk(2) == slice(16, 24)
        assert [p.shape[0] for p in vb.tokens(torch.zeros(24, 3))] == [8, 8, 8]


def test_abi_and_decoder_struct_carry_tok_off():
    with open(os.path.join(ROOT, "include", "factmx.h")) as fp:
        header = fp.read()
    assert nx.ABI_VERSION >= 28 and f"#define FX_ABI_VERSION {nx.ABI_VERSION}" in header
    body = re.search(r"typedef struct fx_decoder_params \{(.*?)\} fx_decoder_params;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.sub(r"[\s\*]", "", d.split()[-1]) for stmt in body.split(";") for d in stmt.split(",") if d.strip()]
    fields = [f[0] for f in nx.DecoderParams._fields_]
    assert names == fields                                   # the same members in the same order
    assert "tok_off" in fields and fields.index("tok_off") == names.index("tok_off")
    assert dict(nx.DecoderParams._fields_)["tok_off"] is ctypes.c_void_p
    assert nx.DecoderParams.tok_off.size == ctypes.sizeof(ctypes.c_void_p)
