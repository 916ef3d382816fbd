"""fx_mha_t_workspace_floats against a plain restatement of the sizing rule of the attention over T
(csrc/attention.cpp tattn_plan, asked without a GPU): the partial workspace of a call is the largest one
any launch plan of its sizes needs -- forward or backward, rows 16-byte aligned or not.

The rule: nvid * nh * nsplit partials of a (Qp x Hp) tile and two rows of Qp each, with
  * the LDS-staged kernels' chunk: the largest power of two in [32, 256] whose LDS images fit, halved while
    the launch has fewer than 256 workgroups; Qp / Hp the queries of a 64-query block / the head dim
    rounded up to 32;
  * the register-resident kernels (head dim 32, <= 32 queries, aligned rows): 32 x 32 tiles and 256-key
    chunks, 128-key chunks when 256 leave fewer than 256 workgroups.
The product covers both sides of the 32- and 64-query edges, of head dim 32, of the 256-workgroup edge of
both chunk rules ((16, 32, 512, 32, 8) against (15, ...)) and of the 16 / 17-chunk edge (T = 4096 / 4097)."""
import itertools

from factmx import native as nx

AT, NVK, QB = 256, 8, 64
NVID = [1, 2, 3, 15, 16, 32]
QV = [1, 8, 31, 32, 33, 64, 65, 70, 128]
TV = [1, 31, 32, 33, 100, 127, 128, 129, 255, 256, 257, 300, 512, 1000, 4095, 4096, 4097, 5000, 8192]
HD = [6, 16, 31, 32, 33, 64]
NH = [1, 2, 4, 8]


def lds_geom(nvid, Qv, Tv, hd, nh, bwd):
    Qp = max(32, (min(Qv, QB) + 31) // 32 * 32)
    Hp = max(32, (hd + 31) // 32 * 32)

    def lds(Tc):
        n = 2 if bwd else 1
        return 4 * (n * Qp * (Hp + 4) + 2 * Tc * (Hp + 4) + n * Qp * (Tc + 4) + 4 * 1024 + 2 * Qp + 4)
    Tc = 256
    while Tc > 32 and (lds(Tc) > 150 * 1024 or Tc * Hp > NVK * 4 * AT or Tc * Qp > 8 * 1024):
        Tc >>= 1
    while Tc > 32 and nvid * nh * ((Tv + Tc - 1) // Tc) < 256:
        Tc >>= 1
    return Qp, Hp, max(1, (Tv + Tc - 1) // Tc)


def rr_tc(nvid, Tv, nh):
    return 256 if nvid * nh * ((Tv + 255) // 256) >= 256 else 128


def ws_floats(nvid, Qv, Tv, hd, nh):
    w = 0
    if hd == 32 and Qv <= 32:
        tc = rr_tc(nvid, Tv, nh)
        n = nvid * nh * ((Tv + tc - 1) // tc)
        w = n * 32 * 32 + 2 * n * 32
    for bwd in (False, True):
        Qp, Hp, nsplit = lds_geom(nvid, Qv, Tv, hd, nh, bwd)
        n = nvid * nh * nsplit
        w = max(w, n * Qp * Hp + 2 * n * Qp)
    return w


def test_workspace_floats_match_the_sizing_rule():
    lib = nx.load()
    shapes = list(itertools.product(NVID, QV, TV, HD, NH))
    assert len(shapes) == 24624          # (nvid = 15: the other side of the 16-video edge)
    bad = [(s, lib.fx_mha_t_workspace_floats(*s), ws_floats(*s)) for s in shapes
           if lib.fx_mha_t_workspace_floats(*s) != ws_floats(*s)]
    assert not bad, (len(bad), bad[:5])
    # the 256-workgroup edge of the register-resident chunk rule lies between 15 and 16 videos of 8 heads
    assert rr_tc(16, 512, 8) == 256 and rr_tc(15, 512, 8) == 128

