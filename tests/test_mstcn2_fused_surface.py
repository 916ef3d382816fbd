"""The fused MS-TCN++ layer's surface (CPU): what the header and the binding declare, the Python switch, and
the size functions under the switch (they launch nothing)."""
import ctypes
import os
import re

import pytest

from factmx import functional as fxf
from factmx import native as nx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "factmx.h")) as fp:
        return fp.read()


def test_header_and_binding_declare_fused_layers_last():
    header = _header()
    assert nx.ABI_VERSION >= 29 and f"#define FX_ABI_VERSION {nx.ABI_VERSION}" in header
    body = re.search(r"typedef struct fx_mstcn2_params \{(.*?)\} fx_mstcn2_params;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.sub(r"[\s\*]", "", d.split()[-1]) for stmt in body.split(";") for d in stmt.split(",") if d.strip()]
    fields = [f[0] for f in nx.Mstcn2Params._fields_]
    assert names == fields                                   # the same members in the same order
    assert fields[-1] == "fused_layers" and dict(nx.Mstcn2Params._fields_)["fused_layers"] is ctypes.c_int
    # the profiler kind of the fused chains is documented, and is none of the X2Y kinds (3-6, 11-14)
    assert nx.PROF_MSTCN2_FUSED == 15 and re.search(r"\b15 = fused MS-TCN\+\+ layer", header)


def test_python_switch_exists_and_reaches_the_params():
    assert isinstance(fxf.MSTCN2_FUSED_LAYERS, int) and fxf.MSTCN2_FUSED_LAYERS in (0, 1, 2)


def _sizes(F, ngroup, fused, rows=111, nl=4):
    lib = nx.load()
    p = nx.Mstcn2Params()
    p.cin, p.F, p.cout, p.num_layers, p.in_map, p.dil_factor = 96, F, 40, nl, 1, 2
    p.ngroup, p.fused_layers = ngroup, fused
    return (lib.fx_mstcn2_saved_floats(ctypes.byref(p), rows), lib.fx_mstcn2_workspace_floats(ctypes.byref(p), rows))


def test_size_functions_reserve_the_superset():
    if not os.path.exists(nx.LIB_PATH):
        pytest.fail("libfactmx.so is not built: the size functions are part of the library")
    for fused in (1, 2):
        s0, w0 = _sizes(256, 1, 0)
        s1, w1 = _sizes(256, 1, fused)
        assert s1 >= s0 and w1 >= w0 and (s1, w1) != (s0, w0)   # room for the fragment-order weights
        assert s1 == s0                                         # the prefix layout of `saved` is what it was
        assert _sizes(512, 1, fused) == _sizes(512, 1, 0)       # F != 256: the GEMM path's sizes
        assert _sizes(256, 4, fused) == _sizes(256, 4, 0)       # grouped convs: the GEMM path's sizes
