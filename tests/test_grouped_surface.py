"""Grouped dilated convolutions (the reference's f_ngp > 1: nn.Conv1d(..., groups=ngroup) in MSTCN /
MSTCN2), checked on CPU (no kernels launched): the modules construct with the reference's parameter
names and shapes, a FACT built from a config with Bi.f_ngp = 2 round-trips its state_dict, and the
library validates ngroup on the host before any HIP call."""
import ctypes
import os
import subprocess

import pytest
import torch
from torch import nn

from factmx import native as nx
from factmx.configs import get_cfg_defaults
from factmx.models.basic import MSTCN, MSTCN2
from factmx.models.blocks import FACT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _RefLayer(nn.Module):
    """reference basic.py:131-145 DilatedResidualLayer, parameters only"""

    def __init__(self, d, F, ln, g):
        super().__init__()
        self.conv_dilated = nn.Conv1d(F, F, 3, padding=d, dilation=d, groups=g)
        self.conv_1x1 = nn.Conv1d(F, F, 1)
        if ln:
            self.norm = nn.LayerNorm(F)


class _RefMSTCN(nn.Module):
    """reference basic.py:173-198 MSTCN, parameters only"""

    def __init__(self, cin, F, cout, nl, ln, g, in_map):
        super().__init__()
        if in_map:
            self.conv_1x1 = nn.Conv1d(cin, F, 1)
        self.layers = nn.ModuleList([_RefLayer(2 ** i, F, ln, g) for i in range(nl)])
        self.conv_out = nn.Conv1d(F, cout, 1)


class _RefMSTCN2(nn.Module):
    """reference basic.py:222-262 MSTCN2, parameters only"""

    def __init__(self, cin, F, cout, nl, g):
        super().__init__()
        self.conv_1x1_in = nn.Conv1d(cin, F, 1)
        self.conv_dilated_1 = nn.ModuleList(
            nn.Conv1d(F, F, 3, padding=2 ** (nl - 1 - i), dilation=2 ** (nl - 1 - i), groups=g) for i in range(nl))
        self.conv_dilated_2 = nn.ModuleList(
            nn.Conv1d(F, F, 3, padding=2 ** i, dilation=2 ** i, groups=g) for i in range(nl))
        self.conv_fusion = nn.ModuleList(nn.Conv1d(2 * F, F, 1) for _ in range(nl))
        self.conv_out = nn.Conv1d(F, cout, 1)


def _shapes(m):
    return [(n, tuple(p.shape)) for n, p in m.named_parameters()]


def test_grouped_modules_construct_with_reference_parameters():
    m = MSTCN(24, 32, 16, 3, ngroup=4, in_map=True)
    assert _shapes(m) == _shapes(_RefMSTCN(24, 32, 16, 3, True, 4, True))
    assert tuple(m.layers[0].conv_dilated.weight.shape) == (32, 8, 3)
    assert m.ngroup == 4 and m.layers[1].ngroup == 4
    m2 = MSTCN2(24, 32, 16, 3, ngroup=2)
    assert _shapes(m2) == _shapes(_RefMSTCN2(24, 32, 16, 3, 2))
    assert tuple(m2.conv_dilated_1[0].weight.shape) == (32, 16, 3)
    assert m2.ngroup == 2
    m.load_state_dict(_RefMSTCN(24, 32, 16, 3, True, 4, True).state_dict(), strict=True)
    m2.load_state_dict(_RefMSTCN2(24, 32, 16, 3, 2).state_dict(), strict=True)


def _tiny_cfg(ngp):
    """A tiny FACT config, set section by section the way helpers.cfg_from_meta does."""
    cfg = get_cfg_defaults()
    over = {
        "FACT": dict(ntoken=8, block="iuUU", fpos=True, cmr=0.0, mwt=0.1),
        "Bi": dict(hid_dim=64, dropout=0.0, a="sca", a_nhead=4, a_ffdim=64, a_layers=2, a_dim=32, f="m", f_layers=3,
                   f_ln=True, f_dim=32, f_ngp=ngp),
        "Bu": dict(f_layers=3, a_nhead=4),
        "BU": dict(f_layers=3, a_nhead=4, s_layers=1),
    }
    for sec, kv in over.items():
        for k, v in kv.items():
            cfg[sec][k] = v
    cfg.TM.use = False
    cfg.holdout_classes = []
    cfg.holdout_mode = False
    cfg.use_clip = False
    return cfg


def test_fact_with_grouped_frame_branch_roundtrips_state_dict():
    torch.manual_seed(0)
    net = FACT(_tiny_cfg(2), 20, 7)
    grouped = [(n, tuple(p.shape)) for n, p in net.named_parameters() if "conv_dilated" in n and n.endswith("weight")]
    assert grouped, "no dilated convs in the tiny model"
    # Bi.f_ngp = 2 reaches every block (Bu / BU inherit f_ngp = None from Bi)
    assert all(s[1] * 2 == s[0] and s[2] == 3 for _, s in grouped), grouped
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    for v in sd.values():
        if v.is_floating_point():
            v.add_(0.25)
    net2 = FACT(_tiny_cfg(2), 20, 7)
    net2.load_state_dict(sd, strict=True)
    for k, v in net2.state_dict().items():
        assert torch.equal(v, sd[k]), k
    dense = FACT(_tiny_cfg(1), 20, 7)
    assert [n for n, _ in dense.named_parameters()] == [n for n, _ in net.named_parameters()]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(nx.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "fact-clip_amd", "csrc"), "-j8"], check=True,
                       stdout=subprocess.DEVNULL)
    return nx.load()


def test_ngroup_validation_without_gpu(lib):
    prm = nx.MstcnParams()
    prm.cin, prm.F, prm.cout, prm.num_layers, prm.layernorm, prm.in_map = 24, 32, 16, 3, 1, 1
    prm.ngroup = 1
    dense = lib.fx_mstcn_saved_floats(ctypes.byref(prm), 200)
    prm.ngroup = 0                      # 0 and 1 both mean dense (zero-initialised structs)
    assert lib.fx_mstcn_saved_floats(ctypes.byref(prm), 200) == dense
    prm.ngroup = 4
    grouped = lib.fx_mstcn_saved_floats(ctypes.byref(prm), 200)
    assert 0 < grouped < dense
    assert dense - grouped == 3 * (3 * 32 * 32 - 3 * 32 * 8)      # the dX-packed conv weights: 3 F cg per layer
    assert lib.fx_conv3g_workspace_floats(200, 32, 4) > 0
    # F = 30 is no multiple of 4 groups: refused before any HIP call (null pointers never read)
    st = lib.fx_conv3g_fwd(None, 30, 64, 64, 1, None, 30, 4, 1, None, None, 0, None, 30, None, None)
    assert st < 0 and b"ngroup" in lib.fx_last_error()
    st = lib.fx_conv3g_bwd(None, 30, 64, 64, 1, None, 30, 4, 1, None, None, 30, None, 30, None, None, None, None)
    assert st < 0 and b"ngroup" in lib.fx_last_error()
    prm.F, prm.ngroup = 30, 4
    st = lib.fx_mstcn_fwd(ctypes.byref(prm), None, 24, 64, 1, None, 16, None, None, None)
    assert st < 0 and b"ngroup" in lib.fx_last_error()
    p2 = nx.Mstcn2Params()
    p2.cin, p2.F, p2.cout, p2.num_layers, p2.in_map, p2.ngroup = 24, 32, 16, 3, 1, -1
    st = lib.fx_mstcn2_fwd(ctypes.byref(p2), None, 24, 64, 1, ctypes.c_void_p(8), 16, ctypes.c_void_p(8),
                           ctypes.c_void_p(8), None)
    assert st < 0 and b"ngroup" in lib.fx_last_error()
