"""fx_x2y_core: which attention core fx_x2y_fwd / fx_x2y_bwd take for given row counts (host only, no
GPU), and the f2a partial slabs of fx_x2y_workspace_floats growing with the query blocks.

The <= 64-row decisions are pinned as they stood before the wide cores (a segment-level f2a call of 103
segments and 32 tokens stays on the f2a core); 65 .. 320 token rows take the wide a2f core when every
video has <= 320 keys, else the wide f2a core when every video has <= 320 queries, else the grouped GEMMs.
Calls of fewer than 1024 rows (segment level) stay on the grouped GEMMs: both wide cores measured slower
than them there (profiles/x2y_tokens.json), and the rule is that such a shape class keeps the grouped path.
"""
import ctypes

import pytest

from factmx import native as nx

HD = 512


@pytest.fixture(scope="module")
def lib():
    return nx.load()


def _offs(counts):
    a = (ctypes.c_int * (len(counts) + 1))()
    for i, c in enumerate(counts):
        a[i + 1] = a[i] + c
    return a


def _core(lib, keys, queries, Hd=HD):
    keys = (keys,) if isinstance(keys, int) else tuple(keys)
    queries = (queries,) if isinstance(queries, int) else tuple(queries)
    assert len(keys) == len(queries)
    xo, yo = _offs(keys), _offs(queries)
    return lib.fx_x2y_core(Hd, len(keys), xo, yo, sum(keys), sum(queries))


@pytest.mark.parametrize("keys,queries,want", [
    (32, 4096, 1),
    (4096, 32, 2),
    (103, 32, 2),        # the segment-level decision as it stood, pinned
    (75, 4096, 1),
    (4096, 75, 2),
    (103, 75, 0),        # segment level: the grouped GEMMs measured faster
    (320, 500, 0),       # likewise
    (500, 320, 0),       # likewise
    (320, 1024, 1),      # the caps at frame level
    (1024, 320, 2),
    (321, 321, 0),
])
def test_core_for_row_counts(lib, keys, queries, want):
    assert _core(lib, keys, queries) == want


def test_ragged_videos_in_one_call(lib):
    # token counts (40, 75) as the keys of two videos: one call, the wide a2f core
    assert _core(lib, (40, 75), (3000, 2000)) == 1
    # and as the queries over frames: the wide f2a core
    assert _core(lib, (3000, 2000), (40, 75)) == 2


def test_single_video_null_offsets(lib):
    assert lib.fx_x2y_core(HD, 1, None, None, 75, 4096) == 1
    assert lib.fx_x2y_core(HD, 1, None, None, 4096, 75) == 2


def test_other_conditions_stay(lib):
    assert _core(lib, (32,) * 17, (100,) * 17) == 0      # 17 videos
    assert _core(lib, (32,) * 16, (100,) * 16) == 1
    assert _core(lib, 32, 4096, Hd=384) == 0             # Hd % 256
    assert _core(lib, 75, 4096, Hd=384) == 0
    assert _core(lib, 32, 4096, Hd=256) == 1
    assert _core(lib, 64 * 1024 + 1, 75) == 0            # more than 1024 key chunks in a video
    assert _core(lib, 64 * 1024, 75) == 2


def test_f2a_workspace_grows_with_query_blocks(lib):
    Nx, xdim, ydim, outdim = 4096, 256, 256, 192
    chunks = Nx // 64

    def ws(nq):
        return lib.fx_x2y_workspace_floats(Nx, xdim, nq, ydim, HD, outdim, 1, None, None)

    # 75 queries: two 64-query blocks of partial rows and stats per chunk instead of one
    assert ws(75) - ws(64) >= chunks * 64 * (HD + 2)
    # 320 queries: five blocks
    assert ws(320) - ws(64) >= chunks * 4 * 64 * (HD + 2)
