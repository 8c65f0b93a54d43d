"""The build unit's handles own their device memory (csrc/mcq_build.hip: Table, Parts, PartsBuilder) and share two host functions:
filter_table behind rank_split / remove_ambiguous, emit_part behind Parts and PartsBuilder.finish.  Small inputs at the edges of
those two -- lists of exactly 1, 17 and 33 locations, a filter that keeps nothing, a filter of an emptied table, a feature-hash
range that receives nothing -- against the NumPy filters of the other tests and against the one-piece build, and a count of the
device memory that stays allocated over repeated build / filter / close cycles."""
import importlib

import numpy as np
import pytest
import torch

import ambig_ref as ar
from oracle import mc_oracle as orc
from test_gpu_build_cli import _numpy_split

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", np.uint8)


@pytest.fixture(scope="module")
def eng():
    return importlib.import_module("metacache-mpi_amd.engine")


def _identical(n, acgt=128):
    """n targets, each the same 128 random bases (one window): every key has a list of exactly n locations.  acgt < 128: only
    that many bases and N after them, so that the window has fewer than 16 features"""
    mer = ACGT[np.random.default_rng(1000 + n).integers(0, 4, 128)].copy()
    mer[acgt:] = ord("N")
    return np.tile(mer, n), np.arange(n + 1, dtype=np.uint64) * np.uint64(128)


def _different(n, length, seed=7):
    return ACGT[np.random.default_rng(seed).integers(0, 4, n * length)], np.arange(n + 1, dtype=np.uint64) * np.uint64(length)


def _range_of(keys, n_ranges):
    """feature-hash range of every key, as mcq_owner and the parts cut them: (thomas_mueller_hash(key) * n_ranges) >> 32"""
    x = keys.astype(np.uint64)
    for _ in range(2):
        x = (((x >> np.uint64(16)) ^ x) * np.uint64(0x45d9f3b)) & np.uint64(0xFFFFFFFF)
    x = (x >> np.uint64(16)) ^ x
    return ((x * np.uint64(n_ranges)) >> np.uint64(32)).astype(np.int64)


def _equal(table, want, win):
    k, o, l, w = table.to_host()
    assert table.n_keys == len(want[0]) and table.n_locs == len(want[2])
    assert np.array_equal(k, want[0]) and np.array_equal(o, want[1]) and np.array_equal(l, want[2]) and np.array_equal(w, win)


PARENT_DRIFT = 0          # bytes; see the assertion of the last test
EMPTY = (np.zeros(0, np.uint32), np.zeros(1, np.uint64), np.zeros(0, np.uint64))


@pytest.mark.parametrize("n,acgt", [(1, 128), (17, 128), (33, 128), (1, 22)])
def test_filters_of_lists_of_one_two_and_three_steps(eng, n, acgt):
    """(a whole window of 128 bases has 16 features, four rounds of a wave's four keys; 22 bases have 7 k-mers: the last round of
    the wave has an idle group)"""
    bases, off = _identical(n, acgt)
    table = eng.Table(bases.ctypes.data, off.ctypes.data, n, device_ptrs=False)
    keys, loff, locs, win = table.to_host()
    assert 0 < table.n_keys <= 16 and np.all(np.diff(loff.astype(np.int64)) == n)
    assert table.n_keys == (16 if acgt == 128 else 7)
    opened = [table]

    def made(t):
        opened.append(t)
        return t
    for P, r in ((2, 0), (2, 1)):
        _equal(made(table.rank_split(P, r)), _numpy_split(keys, loff, locs, P, r), win)
    nothing = made(table.rank_split(64, 40))                     # a rank that owns no target
    _equal(nothing, EMPTY, win)
    same = np.full(n, 5, np.uint32)
    out, removed = table.remove_ambiguous(same, 1)
    _equal(made(out), (keys, loff, locs), win)
    assert removed == 0
    ids = np.arange(n, dtype=np.uint32)
    emptied = None
    for max_keys in (1, 3):
        out, removed = table.remove_ambiguous(ids, max_keys)
        ek, eo, el, want_removed = ar.numpy_filter(keys, loff, locs, ids, max_keys)
        _equal(made(out), (ek, eo, el), win)
        assert removed == want_removed == (table.n_keys if n > max_keys else 0)
        if n > max_keys:
            emptied = out
    # the two filters chained in both orders, on tables that one of them emptied
    for src in (nothing, emptied) if emptied is not None else (nothing,):
        _equal(made(src.rank_split(2, 0)), EMPTY, win)
        out, removed = src.remove_ambiguous(ids, 1)
        _equal(made(out), EMPTY, win)
        assert removed == 0
    half, removed = made(table.rank_split(2, 1)).remove_ambiguous(ids, 3)
    sk, so, sl = _numpy_split(keys, loff, locs, 2, 1)
    ek, eo, el, want_removed = ar.numpy_filter(sk, so, sl, ids, 3)
    _equal(made(half), (ek, eo, el), win)
    assert removed == want_removed
    for t in opened:
        t.close()


@pytest.mark.parametrize("which", ["33-identical", "8-different"])
def test_parts_from_both_builders_equal_the_one_piece_table(eng, which, monkeypatch):
    """mcq_build_parts and a PartsBuilder fed the table's own triples give the database of the one-piece build: emit_part from both
    callers.  The 33 identical targets have at most 16 keys; the number of ranges is the first from 3 up that leaves one empty."""
    dev = torch.device("cuda", 0)
    bases, off = _identical(33) if which == "33-identical" else _different(8, 2000)
    nt = len(off) - 1
    d_bases = torch.from_numpy(bases.copy()).to(dev)
    d_off = torch.from_numpy(off.view(np.int64).copy()).to(dev)
    t2t = np.arange(1, nt + 1, dtype=np.uint32)
    d_t2t = torch.from_numpy(t2t.view(np.int32).copy()).to(dev)
    rng = np.random.default_rng(3)
    reads = []
    for _ in range(64):
        t = int(rng.integers(0, nt))
        length = int(off[t + 1] - off[t])
        n = min(100, length)
        at = int(off[t]) + int(rng.integers(0, length - n + 1))
        reads.append(bases[at:at + n].tobytes())
    rb, ro = orc.pack_reads(reads)

    def answers(db):
        ws = eng.Workspace(db, len(reads), len(rb))
        cands, ncand = ws.query_host(rb, ro, False, max_cand=4)
        ws.close()
        lay = db.layout()
        db.close()
        return {x: lay[x] for x in ("n_keys", "n_locs", "n_windows")}, cands, ncand

    monkeypatch.delenv("MCQ_BUILD_PARTS", raising=False)
    table = eng.Table(d_bases.data_ptr(), d_off.data_ptr(), nt)
    keys, loff, locs, win = table.to_host()
    tw = table.tgt_windows()
    table.close()
    # (the one-piece build in the global-window form of the parts: a handle of bit-field words does not count windows)
    want = answers(eng.Database.build(d_bases.data_ptr(), d_off.data_ptr(), d_t2t.data_ptr(), nt, flags=eng.MCQ_DB_LOCS_GW))
    assert want[0] == {"n_keys": len(keys), "n_locs": len(locs), "n_windows": int(win[-1])} and int((want[2] > 0).sum()) >= 32

    n_ranges = 3
    if which == "33-identical":
        assert len(keys) <= 16
        n_ranges = next(r for r in range(3, 40) if len(set(_range_of(keys, r).tolist())) < r)
    filled = np.bincount(_range_of(keys, n_ranges), minlength=n_ranges)
    assert (filled == 0).any() == (which == "33-identical"), filled
    assert all(orc.tmh(int(k)) * n_ranges >> 32 == r for k, r in zip(keys[:16], _range_of(keys[:16], n_ranges)))
    monkeypatch.setenv("MCQ_BUILD_PARTS", str(n_ranges))

    parts = eng.Parts(d_bases.data_ptr(), d_off.data_ptr(), nt)
    builder = eng.PartsBuilder(tw, expected_locations=len(locs))
    lens = np.diff(loff.astype(np.int64))
    feat, tgt, w = np.repeat(keys, lens), (locs >> np.uint64(32)).astype(np.uint32), (locs & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    cut = len(feat) // 3                                         # (two chunks: the second one grows nothing, the staging arrays do)
    builder.add(feat[:cut], tgt[:cut], w[:cut])
    builder.add(feat[cut:], tgt[cut:], w[cut:])
    streamed = builder.finish()
    for p in (parts, streamed):
        assert (p.n_parts, p.n_keys, p.n_locs, p.n_windows) == (n_ranges, len(keys), len(locs), int(win[-1]))
        got = answers(p.database(d_t2t.data_ptr()))
        p.close()
        assert got[0] == want[0]
        valid = np.arange(want[1].shape[1])[None, :] < want[2][:, None]          # (rows past a read's count are not written)
        assert np.array_equal(got[2], want[2]) and np.array_equal(got[1][valid], want[1][valid])


def _cycle(eng, d_bases, d_off, nt, d_key, d_t2t):
    """one of everything the build unit allocates for a caller, all closed again -> bytes of the smallest per-key array made"""
    table = eng.Table(d_bases.data_ptr(), d_off.data_ptr(), nt)
    split = table.rank_split(2, 0)
    filtered, _ = table.remove_ambiguous(d_key.data_ptr(), 1)
    parts = eng.Parts(d_bases.data_ptr(), d_off.data_ptr(), nt)
    db = parts.database(d_t2t.data_ptr())
    keys, loff, locs, _ = table.to_host()
    builder = eng.PartsBuilder(table.tgt_windows(), expected_locations=table.n_locs)
    builder.add(np.repeat(keys, np.diff(loff.astype(np.int64))), (locs >> np.uint64(32)).astype(np.uint32), (locs & np.uint64(0xFFFFFFFF)).astype(np.uint32))
    streamed = builder.finish()
    assert parts.n_parts == 2 and streamed.n_parts == 2 and streamed.n_keys == parts.n_keys == table.n_keys
    smallest = 4 * min([split.n_keys, filtered.n_keys] + np.bincount(_range_of(keys, 2), minlength=2).tolist())
    for h in (streamed, db, parts, filtered, split, table):
        h.close()
    return smallest


def test_nothing_stays_allocated_over_build_filter_close_cycles(eng, monkeypatch):
    """64 targets of 20 000 random bases: table, rank_split(2, 0), remove_ambiguous(.., 1), Parts in 2 parts, their database, a
    PartsBuilder through finish(), everything closed; one warm-up cycle, then 16, free device memory read after the first and the
    last of them.  The smallest array with one entry per key or per location that a cycle makes (the keys of one part, of one
    rank) is asserted to hold 256 KiB or more, so a member that no destructor reaches costs 4 MiB or more over the 16 cycles.
    (The arrays with one entry per target -- win_off, tgt_windows, the builder's cursors -- hold a few hundred bytes: they sit
    below what free-memory readings resolve and are not what this test sees.)"""
    dev = torch.device("cuda", 0)
    nt = 64
    bases, off = _different(nt, 20000, seed=9)
    d_bases = torch.from_numpy(bases.copy()).to(dev)
    d_off = torch.from_numpy(off.view(np.int64).copy()).to(dev)
    d_key = torch.arange(nt, dtype=torch.int32, device=dev)
    d_t2t = torch.arange(1, nt + 1, dtype=torch.int32, device=dev)
    monkeypatch.setenv("MCQ_BUILD_PARTS", "2")
    cycles = 16

    def free_now():
        torch.cuda.synchronize(dev)
        torch.cuda.empty_cache()
        return torch.cuda.mem_get_info(dev)[0]
    _cycle(eng, d_bases, d_off, nt, d_key, d_t2t)                # warm-up: the runtime's own pools, the code objects
    smallest = _cycle(eng, d_bases, d_off, nt, d_key, d_t2t)
    first = free_now()
    for _ in range(cycles - 1):
        _cycle(eng, d_bases, d_off, nt, d_key, d_t2t)
    last = free_now()
    drift = first - last
    print("smallest per-key array %d bytes, free after cycle 1 %d, after cycle %d %d, drift %d bytes" % (smallest, first, cycles, last, drift))
    assert smallest >= 256 << 10
    # The same body on the parent commit (hand-written frees, no leak on these paths) drifted by PARENT_DRIFT = 0 bytes in each of
    # three runs on an MI355X (smallest array 361 684 bytes).  Allowed is twice that plus one 2 MiB allocation granule = 2 MiB,
    # which must stay below the granule plus half of what one forgotten array of the smallest kind costs over the cycles (4.76 MiB).
    bound = 2 * PARENT_DRIFT + (2 << 20)
    assert bound < (2 << 20) + cycles * smallest // 2
    assert drift <= bound, (drift, bound)

