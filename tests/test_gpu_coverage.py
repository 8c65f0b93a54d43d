"""mcq_coverage_* (csrc/mcq_coverage.hip) on caller-made ranges and count rows against the plain restatement
(tests/coverage_ref.py): the bitmap word for word -- its two guard words included --, the three numbers per target and the count of
refused ranges; and once on the real outputs of mcq_target_hits, handed over on the device."""
import importlib

import numpy as np
import pytest
import torch

import coverage_ref as ref
from golden_util import Fixture
from oracle import dbfile

pytestmark = pytest.mark.gpu

UNUSED = 0xFFFFFFFF
WINDOWS = [1, 31, 32, 33, 64, 65, 4097]        # side by side: segments of 1, 1, 1, 2, 2, 3 and 129 words
N_QUERIES = [0, 1, 63, 64, 65, 257]


def _eng():
    return importlib.import_module("metacache-mpi_amd.engine")


def make_batch(seed, nq, n_slots, cap, windows=WINDOWS):
    """ranges [nq * n_slots, 4] and counts [nq * n_slots, cap]: unused slots, slots with n_win = 0, ranges that begin at window 0, end on
    the last window of their target or lie anywhere, zero counts inside ranges, and non-zero garbage in every word behind n_win"""
    rng = np.random.default_rng(seed)
    n = nq * n_slots
    ranges = np.zeros((n, 4), np.uint32)
    counts = rng.integers(1, 2 ** 32, size=(n, cap), dtype=np.uint64).astype(np.uint32)
    last = len(windows) - 1
    forced = [(0, 0, 1), (last, windows[last] - min(cap, 2), min(cap, 2)), (3, 32, 1), (1, windows[1] - 1, 1), (2, 0, min(cap, 32)), (last, 0, 1)]
    for j in range(n):
        kind = int(rng.integers(0, 10))
        garbage = int(rng.integers(1, 2 ** 32))
        if j < len(forced):
            tgt, beg, n_win = forced[j]
        elif kind == 0:
            ranges[j] = (UNUSED, garbage, int(rng.integers(0, 50)), int(rng.integers(0, cap + 1)))
            continue
        elif kind == 1:
            ranges[j] = (int(rng.integers(0, len(windows))), garbage, int(rng.integers(0, 2 ** 32)), 0)
            continue
        else:
            tgt = int(rng.integers(0, len(windows)))
            W = windows[tgt]
            n_win = int(rng.integers(1, min(cap, W) + 1))
            where = int(rng.integers(0, 3))
            beg = 0 if where == 0 else (W - n_win if where == 1 else int(rng.integers(0, W - n_win + 1)))
        ranges[j] = (tgt, garbage, beg, n_win)
        c = rng.integers(1 if j < len(forced) else 0, 4, size=n_win).astype(np.uint32)   # a quarter of the windows of a range have no match
        if j % 5 == 0:
            c[0] = 0xFFFFFFF0                                                  # sums that need more than 32 bits
        counts[j, :n_win] = c
    return ranges, counts


def on_device(ranges, counts):
    return (torch.from_numpy(ranges.view(np.int32).copy()).cuda(), torch.from_numpy(counts.view(np.int32).copy()).cuda())


def check(cov, want, ctx, scale=1):
    """the device's state against the restatement's; scale: the batches were added that many times"""
    got, oor = cov.read()
    rows = want.read()
    assert got["windows_covered"].tolist() == [r[2] for r in rows], ctx
    assert got["queries"].tolist() == [scale * r[1] for r in rows], ctx
    assert got["hits"].tolist() == [scale * r[0] for r in rows], ctx
    assert oor == scale * want.out_of_range, ctx
    words, off = cov.bitmap()
    assert off.tolist() == want.word_off, ctx
    assert words[0] == 0 and words[-1] == 0, ctx                                # the guards in front of the first and behind the last target
    assert np.array_equal(words[1:-1], want.words), (ctx, np.nonzero(words[1:-1] != want.words)[0][:8])


@pytest.mark.parametrize("n_slots", [1, 2, 16])
@pytest.mark.parametrize("cap", [1, 3, 67])
def test_caller_made_batches(n_slots, cap):
    eng = _eng()
    cov = eng.Coverage(WINDOWS)
    covered_some = False
    for nq in N_QUERIES:
        ranges, counts = make_batch(1000 * n_slots + 10 * cap + nq, nq, n_slots, cap)
        want = ref.RefCoverage(WINDOWS)
        want.add(ranges, counts, cap)
        assert want.out_of_range == 0
        d_rng, d_cnt = on_device(ranges, counts)
        cov.add(d_rng, d_cnt, nq, n_slots, cap)
        check(cov, want, (n_slots, cap, nq))
        # the same batch again: no new bit, queries and hits doubled
        cov.add(d_rng, d_cnt, nq, n_slots, cap)
        check(cov, want, (n_slots, cap, nq, "twice"), scale=2)
        covered_some = covered_some or any(r[2] for r in want.read())
        if nq * n_slots >= 64:                                                  # the inputs hold what the test is about
            rows = want.read()
            assert rows[0][2] == 1 and all(r[1] > 0 for r in rows), (n_slots, cap, nq)
            last = len(WINDOWS) - 1
            assert want.words[want.word_off[last + 1] - 1] == 1                  # window 4096: the last target's last window, alone in its word
            n_win = ranges[:, 3].astype(np.int64)
            live = (ranges[:, 0] != UNUSED) & (n_win > 0)
            inside = np.arange(cap)[None, :] < n_win[:, None]
            assert ((counts == 0) & inside & live[:, None]).any() and (counts[~inside] != 0).all()
            assert (ranges[:, 0] == UNUSED).any() and ((ranges[:, 0] != UNUSED) & (n_win == 0)).any()
        cov.reset()
        check(cov, ref.RefCoverage(WINDOWS), (n_slots, cap, nq, "reset"))
    assert covered_some


def test_many_queries_on_one_window():
    """4096 queries all on window 63 of target 4: one bit, and counters that lose no add"""
    eng = _eng()
    nq, cap = 4096, 3
    ranges = np.tile(np.array([[4, 0, 63, 1]], np.uint32), (nq, 1))
    counts = np.tile(np.array([[5, 0xBAD, 0xBAD]], np.uint32), (nq, 1))
    cov = eng.Coverage(WINDOWS)
    cov.add(*on_device(ranges, counts), nq, 1, cap)
    got, oor = cov.read()
    assert oor == 0
    assert got["queries"].tolist() == [0, 0, 0, 0, nq, 0, 0] and got["hits"].tolist() == [0, 0, 0, 0, 5 * nq, 0, 0]
    assert got["windows_covered"].tolist() == [0, 0, 0, 0, 1, 0, 0]
    want = ref.RefCoverage(WINDOWS)
    want.add(ranges[:1], counts[:1], cap)
    words, _ = cov.bitmap()
    assert np.array_equal(words[1:-1], want.words)


def test_ranges_outside_their_target_are_refused_and_counted():
    eng = _eng()
    cap, n_slots = 3, 2
    n_t = len(WINDOWS)
    bad = [(3, 7, 31, 3),                    # windows 31..33 of a target of 33: one past the end, the next target's first bit
           (0, 7, 1, 1),                     # window 1 of a target of 1
           (2, 7, 32, 1),                    # window 32 of a target of 32: the next segment's first word
           (n_t - 1, 7, 4096, 2),            # behind the last target: the guard word
           (n_t - 1, 7, 0xFFFFFFFF, 1),      # win_beg + n_win wraps in 32 bits
           (n_t, 7, 0, 1),                   # the first id that is no target
           (0x7FFFFFFF, 7, 0, 1),
           (1, 7, 0, cap + 1)]               # wider than a count row
    good = [(3, 7, 30, 3), (0, 7, 0, 1), (2, 7, 31, 1), (n_t - 1, 7, 4095, 2), (5, 7, 62, 3)]
    rows = []
    for i in range(max(len(bad), len(good))):                                  # bad and good slots interleaved, in both slots of a query
        rows += [bad[i % len(bad)], good[i % len(good)]]
    ranges = np.array(rows, np.uint32)
    nq = len(ranges) // n_slots
    counts = np.full((len(ranges), cap), 2, np.uint32)
    want = ref.RefCoverage(WINDOWS)
    want.add(ranges, counts, cap)
    assert want.out_of_range == len(bad) and want.read()[3][2] == 3 and want.read()[0][2] == 1
    cov = eng.Coverage(WINDOWS)
    cov.add(*on_device(ranges, counts), nq, n_slots, cap)
    check(cov, want, "refused")
    # only the refused ones: nothing at all is set
    only = np.array(bad, np.uint32)
    cov.reset()
    cov.add(*on_device(only, np.full((len(only), cap), 2, np.uint32)), len(only), 1, cap)
    got, oor = cov.read()
    assert oor == len(bad) and not got["queries"].any() and not got["hits"].any() and not got["windows_covered"].any()
    assert not cov.bitmap()[0].any()


def test_rejected_arguments():
    eng = _eng()
    with pytest.raises(eng.McqError):
        eng.Coverage([])
    cov = eng.Coverage([5])
    d_rng, d_cnt = on_device(np.array([[0, 1, 0, 1]] * 2, np.uint32), np.ones((2, 1), np.uint32))
    for n_slots, cap in ((0, 1), (1, 0)):
        with pytest.raises(eng.McqError) as e:
            cov.add(d_rng, d_cnt, 1, n_slots, cap)
        assert e.value.code == eng.MCQ_E_ARG
    with pytest.raises(eng.McqError) as e:                                      # ranges are read 16 bytes at a time
        cov.add(d_rng.data_ptr() + 4, d_cnt, 1, 1, 1)
    assert e.value.code == eng.MCQ_E_ARG
    cov.add(None, None, 0, 1, 1)                                                # an empty batch: nothing to name, nothing done
    assert cov.read()[1] == 0 and not cov.read()[0]["queries"].any()


def test_real_outputs_of_target_hits_in_two_batches():
    """mini, paired: every read asks for every target; the ranges and count rows go from mcq_target_hits into mcq_coverage_add on the
    device, batch by batch, and the result is what the restatement makes of those same outputs"""
    eng = _eng()
    host = importlib.import_module("metacache-mpi_amd.host")
    fx = Fixture("mini", 2)
    keys, off, locs = dbfile.union_shards(fx.shards)
    p = fx.params
    db = eng.Database(keys, off, locs, fx.tax.target_keys(fx.n_targets, 0), k=p["qk"], sketch_size=p["qs"], winlen=p["qwinlen"],
                      winstride=p["qwinstride"], tgt_winstride=p["winstride"])
    rdb = host.RefDb(fx.shard_paths[0][: -len(".db_0")], 2)
    windows = rdb.seq_windows()
    n_slots = min(fx.n_targets, 16)
    nq_all = len(fx.names)
    cov = eng.Coverage(windows)
    want = ref.RefCoverage(windows)
    ws = eng.Workspace(db, nq_all, sum(len(a) + len(b) for a, b in zip(fx.r1, fx.r2)) + 64)
    st = torch.cuda.current_stream().cuda_stream
    keep = []
    for lo, hi in ((0, nq_all // 2 + 1), (nq_all // 2 + 1, nq_all)):           # two batches of unequal size
        seqs = [s for a, b in zip(fx.r1[lo:hi], fx.r2[lo:hi]) for s in (a, b)]
        raw = np.frombuffer("".join(seqs).encode(), np.uint8)
        seq_off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
        nq = hi - lo
        cap = ws.target_hits_range_cap(max(len(a) + len(b) for a, b in zip(fx.r1[lo:hi], fx.r2[lo:hi])), 400)
        d_bases = torch.from_numpy(np.concatenate([raw, np.zeros(8, np.uint8)])).cuda()
        d_off = torch.from_numpy(seq_off).cuda()
        d_tgt = torch.from_numpy(np.tile(np.arange(n_slots, dtype=np.int32), (nq, 1))).cuda()
        d_rng = torch.zeros((nq * n_slots, 4), dtype=torch.int32, device="cuda")
        d_cnt = torch.full((nq * n_slots, cap), 0x5EEDFACE, dtype=torch.int32, device="cuda")
        d_st = torch.zeros(nq, dtype=torch.int32, device="cuda")
        ws.target_hits(d_bases.data_ptr(), d_off.data_ptr(), 2 * nq, True, d_tgt.data_ptr(), n_slots, cap, d_rng.data_ptr(), d_cnt.data_ptr(),
                       d_st.data_ptr(), insert_size_max=400, stream=st)
        cov.add(d_rng, d_cnt, nq, n_slots, cap, stream=st)
        keep.append((d_bases, d_off, d_tgt, d_rng, d_cnt, d_st))
        torch.cuda.synchronize()
        assert not d_st.cpu().numpy().any()
        want.add(d_rng.cpu().numpy().view(np.uint32), d_cnt.cpu().numpy().view(np.uint32), cap)
    check(cov, want, "mini")
    rows = want.read()
    assert sum(1 for r in rows if r[2]) >= 2 and sum(r[1] for r in rows) >= nq_all // 2      # the reads do land on several targets
