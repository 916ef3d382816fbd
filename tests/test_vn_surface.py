"""Python surface of the verb/noun FACT (factmx.models.blocks_SepVerbNoun) -- CPU only, no kernels:
parameter layout against the reference capture, state_dict round trip, mapping files, block letters
and the inverse (CSR) lists the backward kernel gathers through."""
import pytest
import torch

from helpers import load_fixture, tiny_meta, cfg_from_meta


@pytest.fixture(scope="module")
def fixture():
    fx = load_fixture("tiny_vn")
    return fx, tiny_meta(fx)


def _build(fx, meta, block=None):
    from factmx.models import blocks_SepVerbNoun as vn
    vn.set_verb_noun_ids(fx["vids"].tolist(), fx["nids"].tolist())
    cfg = cfg_from_meta(meta)
    if block is not None:
        cfg.FACT.block = block
    return vn.FACT(cfg, meta["D"], meta["V"], meta["N"])


def test_parameter_names_order_and_shapes(fixture):
    fx, meta = fixture
    net = _build(fx, meta)
    got = [(n, list(p.shape)) for n, p in net.named_parameters()]
    assert got == [(n, list(s)) for n, s in meta["param_shapes"].items()]
    blk = net.block_list[0]
    assert blk.seg_update.num_layers == 2 and blk.seg_update.bidirectional          # InputBlockTDU's 2-layer BiGRU
    assert net.block_list[1].seg_update.num_layers == meta["BU"]["s_layers"]


def test_transcript_embeddings_surface(fixture):
    fx, meta = fixture
    from factmx.models import blocks_SepVerbNoun as vn
    vn.set_verb_noun_ids(fx["vids"].tolist(), fx["nids"].tolist())
    cfg = cfg_from_meta(meta)
    cfg.FACT.trans = True
    net = vn.FACT(cfg, meta["D"], meta["V"], meta["N"])
    a = cfg.Bi.a_dim
    assert tuple(net.verb_embed.weight.shape) == (meta["V"], a // 2)
    assert tuple(net.noun_embed.weight.shape) == (meta["N"], a // 2)
    assert not hasattr(net, "action_query")


def test_state_dict_round_trip(fixture):
    fx, meta = fixture
    a, b = _build(fx, meta), _build(fx, meta)
    with torch.no_grad():
        for p in a.parameters():
            p.normal_()
    missing, unexpected = b.load_state_dict(a.state_dict(), strict=True)
    assert not missing and not unexpected
    for (n, p), (m, q) in zip(a.state_dict().items(), b.state_dict().items()):
        assert n == m and torch.equal(p, q), n


def test_unknown_block_letter(fixture):
    fx, meta = fixture
    for bad in ("IuU", "iUU", "IUx"):
        with pytest.raises(ValueError):
            _build(fx, meta, block=bad)


def test_load_verb_noun_ids(tmp_path):
    from factmx.models import blocks_SepVerbNoun as vn
    (tmp_path / "verb_mapping.txt").write_text("0 take\n1 put\n2 open\n")
    (tmp_path / "noun_mapping.txt").write_text("0 pan\n1 lid\n2 tap\n3 cupboard\n")
    (tmp_path / "mapping.txt").write_text("0 take,pan\n1 put,lid\n2 open,cupboard\n3 take,lid\n4 open,tap\n")
    m = vn.load_verb_noun_ids(str(tmp_path / "mapping.txt"), str(tmp_path / "verb_mapping.txt"),
                              str(tmp_path / "noun_mapping.txt"))
    assert m.vids == [0, 1, 2, 0, 2]
    assert m.nids == [0, 1, 3, 1, 2]
    assert (m.num_actions, m.num_verbs, m.num_nouns) == (5, 3, 4)
    assert vn.init_VIDS_NIDS() is m          # an installed mapping is kept: no data/ files are read


def test_csr_lists_invert_the_mapping():
    from factmx.functional import VerbNounMap
    vids = [0, 3, 3, 0, 4, 3]          # verbs 1 and 2 own no action
    nids = [2, 0, 1, 2, 0, 1]
    m = VerbNounMap(vids, nids)
    for n1, n2 in ((5, 3), (6, 4)):    # the frame heads, and the token heads with their closing null bins
        voff, vlist, noff, nlist = m.csr_host(n1, n2)
        assert len(voff) == n1 + 1 and len(noff) == n2 + 1 and voff[0] == noff[0] == 0
        assert voff[-1] == noff[-1] == len(vids) == len(vlist) == len(nlist)
        for ids, off, lst, nb in ((vids, voff, vlist, n1), (nids, noff, nlist, n2)):
            for j in range(nb):
                members = lst[off[j]:off[j + 1]]
                assert members == [a for a, i in enumerate(ids) if i == j]      # ascending, complete
        assert voff[1] == voff[2] == voff[3]                                     # the empty verb bins
    with pytest.raises(ValueError):
        m.csr_host(4, 3)               # verb 4 does not fit 4 bins
    with pytest.raises(ValueError):
        VerbNounMap([0, 1], [0])
