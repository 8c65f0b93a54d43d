"""tests/all_hits_ref.py itself (no GPU): the run-length compression of the oracle's match lists on the mini and tie fixtures, and the
two column formatters on hand-written cases."""
import numpy as np
import pytest

import all_hits_ref as ahr
from golden_util import Fixture
from oracle import dbfile
from oracle import mc_oracle as orc


@pytest.mark.parametrize("tag,P", [("mini", 4), ("tie", 2)])
def test_rle_of_the_oracles_match_lists(tag, P):
    fx = Fixture(tag, P)
    keys, off, locs = dbfile.union_shards(fx.shards)
    p = fx.params
    odb = orc.OracleDb(keys, off, locs, fx.tgt2tax(), k=p["qk"], s=p["qs"], winlen=p["qwinlen"], winstride=p["qwinstride"],
                       tgt_winstride=p["winstride"])
    some, merged = 0, 0
    for a, b in zip(fx.r1, fx.r2):
        m = odb.matches(a, b)
        e = ahr.rle(m)
        assert int(e["hits"].sum()) == len(m) and (e["hits"] > 0).all()
        key = (e["tgt"].astype(np.uint64) << np.uint64(32)) | e["win"].astype(np.uint64)
        assert (key[1:] > key[:-1]).all()                       # strictly ascending (target, window)
        assert np.array_equal(np.repeat(key, e["hits"]), m)
        some += len(m) > 0
        merged += len(e) < len(m)
    assert some > len(fx.r1) // 2 and merged > 0                # the fixtures have hits, and hits that share a location


def test_rle_hand_written():
    L = lambda t, w: (t << 32) | w
    e = ahr.rle(np.array([L(0, 5), L(0, 5), L(0, 6), L(2, 0), L(2, 0), L(2, 0), L(0xFFFF, 0xFFFFFFFF)], np.uint64))
    assert e.tolist() == [(0, 5, 2), (0, 6, 1), (2, 0, 3), (0xFFFF, 0xFFFFFFFF, 1)]
    assert len(ahr.rle(np.zeros(0, np.uint64))) == 0
    assert ahr.rle(np.array([L(1, 1)] * 300, np.uint64)).tolist() == [(1, 1, 300)]          # a count beyond 8 bits


def test_all_hits_column():
    names = {0: "seqA", 1: "seqB", 7: "NC_7.1"}
    ent = [(0, 3, 2), (0, 4, 1), (1, 0, 300), (7, 12, 1)]
    # sequence level: name/win:count, one item per (target, window), every item with its comma
    assert ahr.all_hits_column(ent, names, True) == "seqA/3:2,seqA/4:1,seqB/0:300,NC_7.1/12:1,"
    # above: the ancestor's name -- two targets of one species are NOT merged, nor two windows of one target
    species = {0: "Gen one", 1: "Gen one", 7: "NC_7.1"}        # target 7 has no ancestor at the rank: its own name
    assert ahr.all_hits_column(ent, species, False) == "Gen one:2,Gen one:1,Gen one:300,NC_7.1:1,"
    assert ahr.all_hits_column([], names, True) == "" and ahr.all_hits_column([], names, False) == ""
    assert ahr.all_hits_column(ent, names, True, drop={0, 7}) == "seqB/0:300,"
    assert ahr.all_hits_column(ahr.rle(np.array([(1 << 32) | 9] * 2, np.uint64)), names, True) == "seqB/9:2,"


def test_name_of_target_without_an_ancestor():
    """noanc: a target whose lineage has no species -- its own name stands in; at sequence level every target prints its own"""
    fx = Fixture("noanc", 2)
    sp = dbfile.RANK_NAMES.index("species")
    own = [fx.tax.taxa[fx.tax.by_id[-(t + 1)]]["name"] for t in range(fx.n_targets)]
    at_sp = [ahr.name_of_target(fx.tax, t, sp) for t in range(fx.n_targets)]
    assert [ahr.name_of_target(fx.tax, t, 0) for t in range(fx.n_targets)] == own
    without = [t for t in range(fx.n_targets) if fx.tax.lineage[fx.tax.by_id[-(t + 1)], sp] == dbfile.NONE]
    assert without and len(without) < fx.n_targets
    for t in range(fx.n_targets):
        assert (at_sp[t] == own[t]) == (t in without)


def test_locations_column():
    assert ahr.locations_column([], 113, 128) == ""
    assert ahr.locations_column([(0, 0)], 113, 128) == "[0,128] "
    assert ahr.locations_column([(0, 0), (0, 0)], 113, 128) == "[0,128] [0,128] "
    assert ahr.locations_column([(3, 5), (10, 10)], 113, 128) == "[339,693] [1130,1258] "
    assert ahr.locations_column([(1, 2)], 53, 64) == "[53,170] "
