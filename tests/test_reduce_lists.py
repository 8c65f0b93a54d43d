"""The oracle's reduce (rows 8-11 from a caller-made location list) against the plain reference of tests/reduce_lists.py on
the whole adversarial corpus, at P = 1.  No GPU: this is what entitles tests/test_gpu_reduce_edges.py to take the oracle
as its reference on lists that no fixture contains."""
import functools

import numpy as np
import pytest

import reduce_lists as rl
from oracle import mc_oracle as orc


@functools.lru_cache(maxsize=None)
def _world(seq_level):
    w = rl.World(seq_level)
    odb = orc.OracleDb(w.keys, w.off, w.locs, w.tgt2tax, winstride=rl.TGT_STRIDE)
    lists, qlen, what = rl.flatten(rl.corpus(w))
    return w, odb, lists, qlen, what


def test_corpus_is_what_it_claims():
    """both sides of every routing edge, distinct keys on both sides of 64 and 256, every numWindows, every pattern, any
    order -- and every class of the staged reduce non-empty for both word widths"""
    w, _, lists, qlen, what = _world(False)
    T = np.array([len(x) for x in lists])
    assert set(rl.EDGE_T) <= set(T.tolist()) and T.max() == rl.LMAX
    nw = np.array([rl.num_windows_of(q) for q in qlen])
    assert set(nw.tolist()) == set(rl.NUM_WINDOWS) and rl.W_MAX == int(w.tgt_windows.max())
    D = np.array([len(np.unique(x)) for x in lists])
    short = T <= 512
    for small in (True, False):
        for d in rl.EDGE_D:
            assert ((D == d) & short & ((nw <= 8) == small)).any(), (d, small)
    for tag in "abcdefg":
        assert any(s.startswith(tag + ":") for s in what), tag
    unsorted = sum(1 for x in lists if len(x) > 1 and (np.diff(x.astype(np.int64)) < 0).any())
    assert unsorted > len(lists) // 3 and unsorted < len(lists)
    tgts = np.concatenate(lists) >> np.uint64(32)
    assert int(tgts.max()) == rl.N_TARGETS - 1 and int(tgts.min()) == 0
    for b, flags in ((4, 0), (8, 0), (4, rl.FORCE_RAW_SORT)):
        cls = {rl.route(int(t), int(d), int(n), b, flags, "p1") for t, d, n in zip(T, D, nw)}
        want = {"wave-empty", "block-lds", "block-global"} | ({"wave64"} if b == 8 else {"wave16", "wave-raw"}) | \
               ({"wave-dedup-regs", "wave-dedup-weighted"} if b == 4 and not flags else set())
        assert cls == want, (b, flags, cls ^ want)
    assert len(lists) < 1500 and int(T.sum()) < 1 << 21            # a few hundred lists per batch, most of them short
    assert np.median(T) <= 512


@pytest.mark.parametrize("seq_level", [False, True], ids=["plain", "seq-level-taxa"])
@pytest.mark.parametrize("insert_size_max", [0, rl.INSERT_HUGE], ids=["qlen", "insert2^33"])
def test_oracle_reduce_equals_brute_reduce(seq_level, insert_size_max):
    w, odb, lists, qlen, what = _world(seq_level)
    n_full = 0
    for q, lst in enumerate(lists):
        nw = rl.num_windows_of(qlen[q], insert_size_max)
        tc = rl.target_candidates(lst, nw)
        for M in (1, 2, 4, 16):
            bc, bn = rl.brute_reduce(lst, nw, w.tgt2tax, M, _cands=tc)
            oc, on = odb.reduce_query(lst, int(qlen[q]), max_cand=M, emulate_ranks=1, insert_size_max=insert_size_max)
            assert on == bn and np.array_equal(oc[:on], bc), (what[q], q, len(lst), M, oc[:on], bc)
            n_full += bn == M
    assert n_full > len(lists)          # bounded lists that are full: the insert had something to refuse


def test_brute_reduce_on_hand_made_lists():
    """the plain reference itself, on lists small enough to do by hand"""
    t2t = np.array([7, 7, 9], np.uint32)
    L = lambda *tw: np.array([(t << 32) | w for t, w in tw], np.uint64)
    # hits at 5 and 7 are one range at numWindows = 3, two at numWindows = 2 (the first wins)
    c, n = rl.brute_reduce(L((2, 7), (2, 5)), 3, t2t, 4)
    assert n == 1 and c.tolist() == [[9, 2, 5, 7]]
    c, n = rl.brute_reduce(L((2, 7), (2, 5)), 2, t2t, 4)
    assert c.tolist() == [[9, 1, 5, 5]]
    # two ranges of equal count: the first; a later one with more: that one
    c, n = rl.brute_reduce(L((2, 0), (2, 1), (2, 10), (2, 11)), 2, t2t, 4)
    assert c.tolist() == [[9, 2, 0, 1]]
    c, n = rl.brute_reduce(L((2, 0), (2, 1), (2, 10), (2, 11), (2, 11)), 2, t2t, 4)
    assert c.tolist() == [[9, 3, 10, 11]]
    # targets 0 and 1 share taxon 7: the later one replaces the entry only with strictly more hits
    c, n = rl.brute_reduce(L((0, 3), (1, 4)), 2, t2t, 4)
    assert c.tolist() == [[7, 1, 3, 3]]
    c, n = rl.brute_reduce(L((0, 3), (1, 4), (1, 4), (2, 0)), 2, t2t, 4)
    assert c.tolist() == [[7, 2, 4, 4], [9, 1, 0, 0]]
    # a full list takes a new taxon only in front of an entry with strictly fewer hits
    t3 = np.array([1, 2, 3], np.uint32)
    c, n = rl.brute_reduce(L((0, 0), (1, 0), (2, 0)), 2, t3, 2)
    assert c.tolist() == [[1, 1, 0, 0], [2, 1, 0, 0]]
    c, n = rl.brute_reduce(L((0, 0), (1, 0), (2, 0), (2, 0)), 2, t3, 2)
    assert c.tolist() == [[3, 2, 0, 0], [1, 1, 0, 0]]
    assert rl.brute_reduce(np.zeros(0, np.uint64), 3, t3, 2)[1] == 0
