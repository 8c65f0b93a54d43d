"""mcq_table_remove_ambiguous (-remove-ambig-features on the device, csrc/mcq_build.hip) against the NumPy statement of
remove_ambiguous_features (tests/ambig_ref.py: distinct (key index, tgt_key[target]) pairs per key) on Table.to_host().

The synthetic tables hold lists of chosen length: every target is exactly 128 bases, one window.  A group of length m is one
random 128-mer copied into m targets (its <= 16 features get lists of length m), followed by m targets with a private random
128-mer each -- the private 128-mer of every copy, a target of its own so that every target keeps its one window -- whose
features are singletons.  The kernel works in groups of 16 lanes, four keys per wave, 16 locations per step: the lengths sit
at and around one step (15, 16, 17), two steps (33), four (64, 65), the per-rank limit (254) and, with two virtual ranks,
beyond 255 (300)."""
import gzip
import importlib
import os

import numpy as np
import pytest
import torch

import ambig_ref as ar
from golden_util import GOLDEN, Fixture
from oracle import dbfile
from oracle import mc_oracle as orc
from test_gpu_build_cli import _numpy_split

pytestmark = pytest.mark.gpu

SPECIES, GENUS = 4, 6
NONE = 0xFFFFFFFF
LENGTHS = {1: (1, 2, 15, 16, 17, 33, 64, 65, 254), 2: (300,)}


@pytest.fixture(scope="module")
def eng():
    return importlib.import_module("metacache-mpi_amd.engine")


def _synthetic(eng, P):
    """the table of LENGTHS[P] built with emulate_ranks = P -> (Table, host arrays, [targets of every shared list])"""
    rng = np.random.default_rng(100 + P)
    acgt = np.frombuffer(b"ACGT", np.uint8)

    def mer():
        return acgt[rng.integers(0, 4, 128)].tobytes()
    seqs, lists = [], []
    for m in LENGTHS[P]:
        shared = mer()
        lists.append(np.arange(len(seqs), len(seqs) + m))
        seqs += [shared] * m + [mer() for _ in range(m)]
    # the number of keys must not be a multiple of 4 (a wave's last round then has idle groups), and whole 128-mers bring 16 features
    # each: one more target of 128 bases has 18 bases and 110 N, three k-mers.  Counted here from the oracle's sketches.
    seqs.append(mer()[:18] + b"N" * 110)
    feats = set()
    for s in set(seqs):
        feats.update(int(f) for f in orc.sketch(s))
    assert len(feats) % 4 != 0
    off = np.arange(len(seqs) + 1, dtype=np.uint64) * np.uint64(128)
    host = np.frombuffer(b"".join(seqs), np.uint8).copy()
    table = eng.Table(host.ctypes.data, off.ctypes.data, len(seqs), emulate_ranks=P, device_ptrs=False)
    arrays = table.to_host()
    assert table.n_keys == len(feats) and table.n_keys % 4 != 0
    lens = np.diff(arrays[1].astype(np.int64))
    assert set(LENGTHS[P]) <= set(lens.tolist()) and (lens == 1).sum() > 100
    assert np.array_equal(table.tgt_windows(), np.ones(len(seqs), np.uint32))
    return table, arrays, lists


_tables = {}


@pytest.fixture(scope="module")
def synthetic(eng):
    def get(P):
        if P not in _tables:
            _tables[P] = _synthetic(eng, P)
        return _tables[P]
    yield get
    for t, _, _ in _tables.values():
        t.close()
    _tables.clear()


def _check(table, arrays, tgt_key, max_keys, device=False, split=None):
    """remove_ambiguous equals the NumPy filter bit for bit; returns (n_removed, keys left)"""
    keys, off, locs, win = arrays
    tgt_key = np.ascontiguousarray(tgt_key, np.uint32)
    ek, eo, el, removed = ar.numpy_filter(keys, off, locs, tgt_key, max_keys)
    if device:
        d = torch.from_numpy(tgt_key.view(np.int32).copy()).to(torch.device("cuda", 0))
        out, n = table.remove_ambiguous(d.data_ptr(), max_keys)
    else:
        out, n = table.remove_ambiguous(tgt_key, max_keys)
    k2, o2, l2, w2 = out.to_host()
    assert n == removed and out.n_keys == len(ek) and out.n_locs == len(el), (max_keys, n, removed)
    assert k2.dtype == np.uint32 and o2.dtype == np.uint64 and l2.dtype == np.uint64
    assert np.array_equal(k2, ek) and np.array_equal(o2, eo) and np.array_equal(l2, el), max_keys
    assert np.array_equal(w2, win)
    assert np.array_equal(out.tgt_windows(), table.tgt_windows())
    for P, r in (split or ()):
        part = out.rank_split(P, r)
        pk, po, pl, pw = part.to_host()
        part.close()
        sk, so, sl = _numpy_split(k2, o2, l2, P, r)
        assert np.array_equal(pk, sk) and np.array_equal(po, so) and np.array_equal(pl, sl) and np.array_equal(pw, win), (P, r)
    out.close()
    return removed, len(ek)


def _list_lengths_left(arrays, tgt_key, max_keys):
    keys, off, locs, _ = arrays
    return set(np.diff(ar.numpy_filter(keys, off, locs, np.asarray(tgt_key, np.uint32), max_keys)[1].astype(np.int64)).tolist())


@pytest.mark.parametrize("device", [False, True], ids=["host-keys", "device-keys"])
@pytest.mark.parametrize("max_keys", [1, 2, 3])
def test_equal_keys_remove_nothing_and_target_ids_remove_the_lists_longer_than_n(eng, synthetic, max_keys, device):
    table, arrays, lists = synthetic(1)
    nt = table.n_targets
    removed, _ = _check(table, arrays, np.full(nt, 7, np.uint32), max_keys, device, split=[(1, 0), (3, 1)])
    assert removed == 0
    removed, left = _check(table, arrays, np.arange(nt, dtype=np.uint32), max_keys, device, split=[(1, 0), (3, 2)])
    assert removed > 0 and left > 0
    assert _list_lengths_left(arrays, np.arange(nt), max_keys) == {m for m in LENGTHS[1] if m <= max_keys} | {1}


def test_exact_up_to_255_distinct_keys(eng, synthetic):
    """the list of 300 targets (two virtual ranks) names 255 distinct keys under t % 255 and 256 under t % 256: with max_keys = 255
    it stays under the first and goes under the second"""
    table, arrays, lists = synthetic(2)
    t = np.arange(table.n_targets, dtype=np.uint32)
    assert len(lists[0]) == 300 and len(np.unique(t[lists[0]] % 255)) == 255 and len(np.unique(t[lists[0]] % 256)) == 256
    removed, _ = _check(table, arrays, t % 255, 255, split=[(2, 0), (2, 1)])
    assert removed == 0 and 300 in _list_lengths_left(arrays, t % 255, 255)
    removed, _ = _check(table, arrays, t % 256, 255, device=True)
    assert removed > 0 and 300 not in _list_lengths_left(arrays, t % 256, 255)
    for max_keys in (1, 2, 254):
        _check(table, arrays, t % 255, max_keys)
        _check(table, arrays, t, max_keys, device=True)


@pytest.mark.parametrize("max_keys", [1, 2, 3])
@pytest.mark.parametrize("where", ["last", "position16"])
def test_the_key_that_makes_a_list_ambiguous_sits_on_one_target_only(eng, synthetic, max_keys, where):
    """the targets of a list cycle through max_keys keys; one more key belongs only to the list's last target, or only to the
    target at position 16 (the first location of the second step)"""
    for P in (1, 2):
        table, arrays, lists = synthetic(P)
        key = np.arange(table.n_targets, dtype=np.uint32) + np.uint32(1 << 20)
        hit = 0
        for g, S in enumerate(lists):
            key[S] = 1000 * g + np.arange(len(S)) % max_keys
            at = len(S) - 1 if where == "last" else 16
            if max_keys <= at < len(S):
                key[S[at]] = 1000 * g + 999
                hit += 1
        assert hit >= (1 if P == 2 else 4)
        _check(table, arrays, key, max_keys, split=[(P, P - 1)])
        left = _list_lengths_left(arrays, key, max_keys)
        for S in lists:                           # (the lengths from 2 up are one list length each; singletons always stay)
            at = len(S) - 1 if where == "last" else 16
            if len(S) >= 2:
                assert (len(S) in left) == (not (max_keys <= at < len(S))), (len(S), left)
        key2 = key.copy()                         # ... and without that key every list stays
        for g, S in enumerate(lists):
            key2[S] = 1000 * g + np.arange(len(S)) % max_keys
        assert _list_lengths_left(arrays, key2, max_keys) >= {len(S) for S in lists}
        _check(table, arrays, key2, max_keys, device=True)


def test_equal_keys_on_targets_that_are_not_adjacent_count_once(eng, synthetic):
    """A, B, A, B, ...: two keys however long the list; A, B, A, C, A, B, A, C: three"""
    for P in (1, 2):
        table, arrays, lists = synthetic(P)
        key = np.arange(table.n_targets, dtype=np.uint32) + np.uint32(1 << 20)
        for g, S in enumerate(lists):
            key[S] = 10 * g + np.arange(len(S)) % 2
        assert _list_lengths_left(arrays, key, 2) >= {len(S) for S in lists}
        removed2, _ = _check(table, arrays, key, 2)
        removed1, _ = _check(table, arrays, key, 1)
        assert removed2 == 0 and removed1 > 0
        for g, S in enumerate(lists):
            key[S] = 10 * g + np.array([0, 1, 0, 2])[np.arange(len(S)) % 4]
        for max_keys in (1, 2, 3):
            _check(table, arrays, key, max_keys, device=True)
        assert _list_lengths_left(arrays, key, 3) >= {len(S) for S in lists}
        assert not _list_lengths_left(arrays, key, 2) & {len(S) for S in lists if len(S) >= 4}


def test_the_none_key_is_a_key_like_any_other(eng, synthetic):
    """two targets without an ancestor share a list: one value (std::set<const taxon*> holding nullptr), the list stays at 1"""
    table, arrays, lists = synthetic(1)
    key = np.arange(table.n_targets, dtype=np.uint32)
    pair = lists[LENGTHS[1].index(2)]
    key[pair] = NONE
    assert 2 in _list_lengths_left(arrays, key, 1) and 2 not in _list_lengths_left(arrays, np.arange(table.n_targets), 1)
    _check(table, arrays, key, 1)
    _check(table, arrays, key, 1, device=True)
    fifteen = lists[LENGTHS[1].index(15)]                        # NONE next to another key: two values
    key[fifteen] = 5
    assert 15 in _list_lengths_left(arrays, key, 1)
    key[fifteen[7]] = NONE
    assert 15 not in _list_lengths_left(arrays, key, 1) and 15 in _list_lengths_left(arrays, key, 2)
    _check(table, arrays, key, 1)
    _check(table, arrays, key, 2)
    assert _check(table, arrays, np.full(table.n_targets, NONE, np.uint32), 1)[0] == 0
    assert _check(table, arrays, np.full(table.n_targets, NONE, np.uint32), 2, device=True)[0] == 0


def test_argument_errors_and_empty_tables(eng, synthetic):
    table, arrays, lists = synthetic(1)
    nt = table.n_targets
    key = np.arange(nt, dtype=np.uint32)
    for args in ((None, 1), (key, 0), (key, 256), (key[:-1], 1), (np.append(key, key[:1]), 1)):
        with pytest.raises(eng.McqError) as e:
            table.remove_ambiguous(*args)
        assert e.value.code == eng.MCQ_E_ARG, args[1]
    assert b"max_keys" in eng.lib().mcq_build_last_error() or b"n_targets" in eng.lib().mcq_build_last_error()
    # every key ambiguous: two targets with the same 128-mer and nothing else
    rng = np.random.default_rng(5)
    mer = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 128)]
    host = np.concatenate([mer, mer])
    off = np.array([0, 128, 256], np.uint64)
    two = eng.Table(host.ctypes.data, off.ctypes.data, 2, device_ptrs=False)
    assert two.n_keys > 0 and _check(two, two.to_host(), [0, 0], 1)[0] == 0
    out, n = two.remove_ambiguous(np.array([0, 1], np.uint32), 1)
    assert n == two.n_keys and out.n_keys == 0 and out.n_locs == 0
    k, o, l, w = out.to_host()
    assert len(k) == 0 and len(l) == 0 and np.array_equal(o, np.zeros(1, np.uint64)) and np.array_equal(w, two.to_host()[3])
    again, n2 = out.remove_ambiguous(np.array([0, 1], np.uint32), 3)       # an empty input gives an empty output
    assert n2 == 0 and again.n_keys == 0 and np.array_equal(again.to_host()[1], np.zeros(1, np.uint64))
    part = out.rank_split(2, 1)
    assert part.n_keys == 0 and part.n_locs == 0
    for t in (part, again, out, two):
        t.close()


def test_species_model_equals_the_numpy_filter(eng):
    """3000 genomes in species of 10 (mutated copies: most features of a genome are shared inside its species, some across), P = 1,
    3 and 64, keys t // 10 (the species) and t // 100"""
    synth = importlib.import_module("metacache-mpi_amd.synth")
    dev = torch.device("cuda", 0)
    gb, goff, _ = synth.make_genomes(300, 10, 2000, 3000, 0.02, seed=11, device=dev)
    nt = goff.numel() - 1
    assert nt == 3000
    t = np.arange(nt, dtype=np.uint32)
    for P in (1, 3, 64):
        table = eng.Table(gb.data_ptr(), goff.data_ptr(), nt, emulate_ranks=P, device=0)
        arrays = table.to_host()
        assert table.n_keys > 100000
        for div in (10, 100):
            for max_keys in (1, 2):
                removed, left = _check(table, arrays, t // div, max_keys, device=(div == 100), split=[(P, P // 2)] if max_keys == 1 else None)
                if div == 10 and max_keys == 1:
                    assert removed > 0 and left > 0, (P, removed, left)
        table.close()


def _load_genomes(tag, dev):
    seqs = []
    with gzip.open(os.path.join(GOLDEN, tag, "genomes.fa.gz"), "rt") as f:
        for line in f:
            if not line.startswith(">"):
                seqs.append(line.strip().encode())
    off = np.zeros(len(seqs) + 1, np.int64); off[1:] = np.cumsum([len(s) for s in seqs])
    bases = torch.from_numpy(np.frombuffer(b"".join(seqs), dtype=np.uint8).copy()).to(dev)
    return bases, torch.from_numpy(off).to(dev)


def test_queries_on_a_filtered_table_get_the_oracles_candidates(eng):
    """mini at P = 4: the table built from the fixture's genomes (the union of the golden shards), filtered on the device with the
    species keys, N = 1, made a queryable handle from the device arrays; the fixture's 197 read pairs get the candidates the
    oracle finds in the NumPy-filtered arrays.  The counts were computed on the CPU from the golden shards with that filter and
    the oracle."""
    host = importlib.import_module("metacache-mpi_amd.host")
    dev = torch.device("cuda", 0)
    fx, P = Fixture("mini", 4), 4
    keys, off, locs = dbfile.union_shards(fx.shards)
    rdb = host.RefDb(fx.shard_paths[0][: -len(".db_0")], P)
    bases, goff = _load_genomes("mini", dev)
    table = eng.Table(bases.data_ptr(), goff.data_ptr(), goff.numel() - 1, emulate_ranks=P)
    arrays = table.to_host()
    assert np.array_equal(arrays[0], keys) and np.array_equal(arrays[1], off) and np.array_equal(arrays[2], locs) and len(keys) == 11327
    species = rdb.clade_keys(SPECIES)
    for tgt_key, max_keys, want in ((species, 1, 798), (species, 2, 182), (rdb.clade_keys(GENUS), 1, 200),
                                    (np.arange(fx.n_targets, dtype=np.uint32), 2, 1857)):
        assert _check(table, arrays, tgt_key, max_keys, split=[(P, 1)])[0] == want
    out, removed = table.remove_ambiguous(species, 1)
    assert removed == 798
    p = fx.params
    kw = dict(k=p["qk"], winlen=p["qwinlen"], winstride=p["qwinstride"], tgt_winstride=p["winstride"])
    t2t = np.asarray(fx.tgt2tax(), np.uint32)
    d_t2t = torch.from_numpy(t2t.view(np.int32).copy()).to(dev)
    db = eng.Database(None, None, None, None, sketch_size=p["qs"], device_ptrs=dict(
        keys=out.keys_ptr, list_off=out.list_off_ptr, locs=out.locs_ptr, tgt2tax=d_t2t.data_ptr(), n_keys=out.n_keys, n_locs=out.n_locs,
        n_targets=fx.n_targets), **kw)
    fk, fo, fl, _ = ar.numpy_filter(keys, off, locs, species, 1)
    odb = orc.OracleDb(fk, fo, fl, t2t, s=p["qs"], **kw)
    plain = orc.OracleDb(keys, off, locs, t2t, s=p["qs"], **kw)
    rb, ro = orc.pack_reads(fx.interleaved())
    ws = eng.Workspace(db, len(fx.names), len(rb))
    assert len(fx.names) == 197
    for ranks in (1, P):
        gc, gn = ws.query_host(rb, ro, True, max_cand=fx.maxcand, emulate_ranks=ranks)
        wc, wn = odb.query(rb, ro, True, max_cand=fx.maxcand, emulate_ranks=ranks)
        assert np.array_equal(gn, wn), np.nonzero(gn != wn)[0][:8]
        mask = np.arange(gc.shape[1])[None, :] < wn[:, None]
        assert np.array_equal(gc[mask], wc[mask])
        uc, un = plain.query(rb, ro, True, max_cand=fx.maxcand, emulate_ranks=ranks)
        other = sum(1 for q in range(197) if un[q] != wn[q] or not np.array_equal(uc[q, :un[q]], wc[q, :wn[q]]))
        assert other == 104 and int((wn > 0).sum()) == 194, (ranks, other, int((wn > 0).sum()))
    ws.close()
    db.close()
    out.close()
    table.close()
