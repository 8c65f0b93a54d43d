"""The lean first wave stage's probe: a bucket's head in one 16-B load -- key, list length and the two offset words together -- in
the single unpacked instantiations.  MCQ_FORCE_LEAN_WAVE against MCQ_FORCE_FULL_WAVE (which keeps the
narrowed loads) and the CPU oracle with test_gpu_lean_loop's comparison: candidates below n_cand, n_cand, and every counter of
mcq_stats.  The batches are laid out for a first stage that takes its reads two by two as well (section 33 tried that on top and
left it out; a build with it passed this file), so neighbours (2j, 2j + 1) come in every combination.

Tables: that file's SMALL and NINE, and both built dense (MCQ_SLOTS_PER_KEY = 1: between one and two slots per key), so that
walks of three and more buckets occur.  No entry point returns a table's slot array, so the walks are restated on the host from
what decides them: a linear-probing table's set of occupied slots does not depend on the order of the inserts, and a feature that
is not in the table walks from its home slot to the first free one.  The test counts those walks among the batch's features and
fails when none is three buckets long (a feature that is in the table may walk as far, which the count leaves out).

A batch is a row of neighbours (2j, 2j + 1):
  lengths   every ordered pair of 100, 128, 129, 150, 160, 161 and 300 bases; 129..160 is what the one-pass sketch takes, so the
            neighbours come as (in, in), (in, out), (out, in) and (out, out)
  kinds     a read of only N (no feature), a read foreign to the table (no location), a read of more than 256 locations (handed
            to the queues), a read with a list that is not inline (more than 14 locations in one list), reads of at most 64 and
            of more than 64 distinct keys; each as the first of two, as the second, and as both, beside an ordinary read
  the rest  the table's ordinary reads, every seventh of them of another length
Batch sizes around the stride of a grid of W waves taking reads two by two: 1, 2, 3, 5, 2 W - 1, 2 W, 2 W + 1 and 6 W + 5, through
device buffers sized exactly, with guard words behind them (MCQ_WAVE_BLOCKS_PER_CU = 1: W = 4 x compute units)."""
import importlib
import os

import numpy as np
import pytest
import torch

from oracle import mc_oracle as orc

import test_gpu_lean_loop as ll

LENGTHS = (100, 128, 129, 150, 160, 161, 300)
INLINE_MAX = 14                     # the longest list a 64-B bucket holds beside its key
ACGT = np.frombuffer(b"ACGT", np.uint8)
N_OPT = 1001                        # reads of the option and dense-table cases (odd: the last read has no neighbour)


def one_pass(n):
    return 129 <= n <= 160


def features_of(read):
    """the read's features, window by window (what the first stage probes)"""
    out = [orc.sketch(read[b:e]) for b, e in orc.windows(len(read), ll.WINLEN, ll.STRIDE)]
    return np.concatenate(out) if out else np.zeros(0, np.uint32)


def tmh_np(x):
    x = np.atleast_1d(np.asarray(x, np.uint32))             # (arrays wrap silently, as the hash does)
    x = ((x >> np.uint32(16)) ^ x) * np.uint32(0x45d9f3b)
    x = ((x >> np.uint32(16)) ^ x) * np.uint32(0x45d9f3b)
    return (x >> np.uint32(16)) ^ x


def occupied_slots(keys, n_slots):
    """which slots of a linear-probing table of n_slots (a power of two, more than len(keys)) hold a key, whatever the order of
    the inserts: slot i is taken when the keys at home in i and those pushed on from the slots before it are at least one
    (Lindley's recursion over the ring, run twice round so that what wraps is in)"""
    assert n_slots & (n_slots - 1) == 0 and len(keys) < n_slots
    c = np.bincount(tmh_np(keys) & np.uint32(n_slots - 1), minlength=n_slots).astype(np.int64)
    c2 = np.concatenate([c, c])
    s = np.cumsum(c2 - 1)
    q = s - np.minimum.accumulate(np.minimum(s, 0))            # keys waiting behind slot i
    q_before = np.concatenate([[0], q[:-1]])
    occ = (q_before + c2 > 0)[n_slots:]
    assert int(occ.sum()) == len(keys)
    return occ


def miss_walks(keys, n_slots, feats):
    """buckets read by the probe of every feature that is not among keys: home slot up to and with the first free one"""
    occ = occupied_slots(keys, n_slots)
    free = np.nonzero(~occ)[0]
    absent = feats[~np.isin(feats, keys)]
    home = (tmh_np(absent) & np.uint32(n_slots - 1)).astype(np.int64)
    nxt = np.searchsorted(free, home)                          # the first free slot at or behind home, round the ring
    dist = np.where(nxt < len(free), free[np.minimum(nxt, len(free) - 1)] - home, free[0] + n_slots - home)
    return dist + 1


def test_walks_restated():
    """the host's count of walks on a table small enough to insert key by key (no GPU in it)"""
    rng = np.random.default_rng(5)
    keys = np.unique(rng.integers(0, 1 << 32, 900, dtype=np.uint64).astype(np.uint32))
    assert [int(v) for v in tmh_np(keys[:9])] == [orc.tmh(int(k)) for k in keys[:9]]
    n_slots = 1024
    table = np.full(n_slots, -1, np.int64)
    for k in rng.permutation(keys):
        i = orc.tmh(int(k)) & (n_slots - 1)
        while table[i] >= 0:
            i = (i + 1) & (n_slots - 1)
        table[i] = int(k)
    assert np.array_equal(table >= 0, occupied_slots(keys, n_slots))
    feats = rng.integers(0, 1 << 32, 500, dtype=np.uint64).astype(np.uint32)
    feats = feats[~np.isin(feats, keys)]
    want = []
    for f in feats:
        i, n = orc.tmh(int(f)) & (n_slots - 1), 1
        while table[i] >= 0:
            i, n = (i + 1) & (n_slots - 1), n + 1
        want.append(n)
    assert np.array_equal(miss_walks(keys, n_slots, feats), np.array(want))
    assert max(want) >= 3


def cut(genome, rng, n):
    at = int(rng.integers(0, len(genome) - n))
    return genome[at:at + n].tobytes()


def neighbours(ordinary, kinds, genome, rng, n_seqs):
    """the batch's reads.  ordinary: reads of 150 bases with locations; kinds: name -> read; genome: where reads of other lengths
    are cut from"""
    out = []
    for la in LENGTHS:
        for lb in LENGTHS:
            out += [cut(genome, rng, la), cut(genome, rng, lb)]
    plain = ordinary[0]
    for r in kinds.values():
        out += [r, plain, plain, r, r, r]
    i = 0
    while len(out) < n_seqs:
        out.append(cut(genome, rng, LENGTHS[(i // 7) % len(LENGTHS)]) if i % 7 == 6 else ordinary[i % len(ordinary)])
        i += 1
    return out[:n_seqs]


def list_lengths(keys, off):
    return dict(zip(keys.tolist(), np.diff(off.astype(np.int64)).tolist()))


def pick_kinds(odb, pool, lens, want):
    """name -> a read of the pool of that kind, by the oracle's matches and the table's list lengths"""
    T, D = ll.kinds_of(odb, pool)
    longest = np.array([max([lens.get(int(f), 0) for f in features_of(r)] or [0]) for r in pool])
    tests = dict(only_n=lambda i: pool[i] == b"N" * ll.READ,
                 foreign=lambda i: T[i] == 0 and len(features_of(pool[i])) > 0,
                 handed_on=lambda i: ll.KEEP_LEAN < T[i] <= ll.KEEP_FULL,
                 external=lambda i: 0 < T[i] <= ll.KEEP_LEAN and longest[i] > INLINE_MAX,
                 few_keys=lambda i: 0 < T[i] <= ll.KEEP_LEAN and D[i] <= 64,
                 many_keys=lambda i: T[i] <= ll.KEEP_LEAN and D[i] > 64)
    out = {}
    for name in want:
        hit = [i for i in range(len(pool)) if tests[name](i)]
        assert hit, "no %s read in the pool" % name
        out[name] = pool[hit[0]]
    return out


def dense(make):
    """the table make() builds with the fewest slots per key"""
    old = os.environ.get("MCQ_SLOTS_PER_KEY")
    os.environ["MCQ_SLOTS_PER_KEY"] = "1"            # read when a table is created
    try:
        return make()
    finally:
        if old is None:
            del os.environ["MCQ_SLOTS_PER_KEY"]
        else:
            os.environ["MCQ_SLOTS_PER_KEY"] = old


@pytest.fixture(scope="module")
def world():
    eng = importlib.import_module("metacache-mpi_amd.engine")
    dbbuild = importlib.import_module("dbbuild_torch")
    synth = importlib.import_module("metacache-mpi_amd.synth")
    dev = torch.device("cuda", 0)
    W = 4 * torch.cuda.get_device_properties(dev).multi_processor_count
    n_seqs = 6 * W + 5
    host = lambda t, ty: t.cpu().numpy().astype(ty)
    rng = np.random.default_rng(71)
    only_n, foreign = b"N" * ll.READ, ACGT[np.random.default_rng(72).integers(0, 4, ll.READ)].tobytes()
    # SMALL: reads drawn like the benchmark's; its lists are short (no list behind the buckets, no read of more than 256 locations)
    gb, goff, species = synth.make_genomes(6, 4, 150_000, 300_000, 0.02, seed=31, device=dev)
    keys, off, locs, _ = dbbuild.build_table(gb, goff, emulate_ranks=2)
    hk, ho = host(keys, np.uint32), host(off, np.uint64)
    odb = orc.OracleDb(hk, ho, host(locs, np.uint64), host(species, np.uint32))
    rd, _, _ = synth.sample_reads(gb, goff, 4096, ll.READ, 0.005, 0.001, seed=91)
    ordinary = [r.tobytes() for r in rd.cpu().numpy().reshape(4096, ll.READ)]
    kinds = pick_kinds(odb, [only_n, foreign] + ordinary[:64], list_lengths(hk, ho), ("only_n", "foreign", "few_keys"))
    genome = host(gb, np.uint8)[:int(goff[1])]
    reads = neighbours(ordinary, kinds, genome, rng, n_seqs)
    small = ll.Table(dbbuild.make_database(keys, off, locs, species), odb, reads)
    small_dense = ll.Table(dense(lambda: dbbuild.make_database(keys, off, locs, species)), odb, reads[:N_OPT])
    small_dense.keys = hk
    # NINE: every kind of read
    g9, at4, at8 = ll.nine_genome(93)
    k9, o9, l9, t9 = ll.nine_table(g9)
    pool = [only_n, foreign] + ll.nine_reads(g9, at4, at8, 94)
    odb9 = orc.OracleDb(k9, o9, l9, t9)
    kinds9 = pick_kinds(odb9, pool, list_lengths(k9, o9), ("only_n", "foreign", "handed_on", "external", "few_keys", "many_keys"))
    reads9 = neighbours(pool[2:], kinds9, np.frombuffer(g9, np.uint8), rng, n_seqs)
    nine = ll.Table(eng.Database(k9, o9, l9, t9), odb9, reads9)
    nine_dense = ll.Table(dense(lambda: eng.Database(k9, o9, l9, t9)), odb9, reads9[:N_OPT])
    nine_dense.keys = k9
    for t in (small, nine):         # the four kinds of neighbours are in every batch of a hundred reads
        n = np.diff(t.off[:99].astype(np.int64))
        assert {(one_pass(a), one_pass(b)) for a, b in zip(n[0::2], n[1::2])} == {(x, y) for x in (False, True) for y in (False, True)}
    old = os.environ.get("MCQ_WAVE_BLOCKS_PER_CU")
    os.environ["MCQ_WAVE_BLOCKS_PER_CU"] = "1"           # read when a workspace is created
    try:
        yield dict(eng=eng, dev=dev, W=W, small=small, nine=nine, small_dense=small_dense, nine_dense=nine_dense,
                   keep=(gb, keys, off, locs, species))
    finally:
        if old is None:
            del os.environ["MCQ_WAVE_BLOCKS_PER_CU"]
        else:
            os.environ["MCQ_WAVE_BLOCKS_PER_CU"] = old


@pytest.mark.gpu
@pytest.mark.parametrize("table", ["small", "nine"])
def test_batch_sizes_around_the_pairs(world, table):
    """one read; one pair; a pair and a read; fewer pairs than waves; one wave without a pair, with half a pair, every wave with
    one, one more read; three rounds and five reads"""
    w = world
    tab, W = w[table], w["W"]
    for nq in (1, 2, 3, 5, 2 * W - 1, 2 * W, 2 * W + 1, 6 * W + 5):
        ll._check(w, tab, nq, False, ll._device_run(w, tab, nq, False, 2, 2, 0), "%s, %d reads" % (table, nq))


@pytest.mark.gpu
@pytest.mark.parametrize("ism", [0, 300])
@pytest.mark.parametrize("P", [1, 2, 3])
@pytest.mark.parametrize("M", [1, 2, 4])
@pytest.mark.parametrize("table", ["small", "nine"])
def test_options(world, table, M, P, ism):
    w = world
    tab = w[table]
    ll._check(w, tab, N_OPT, False, ll._host_run(w, tab, N_OPT, False, M, P, ism), "%s, M %d P %d insert_size_max %d" % (table, M, P, ism),
              M=M, P=P, ism=ism)


@pytest.mark.gpu
@pytest.mark.parametrize("table", ["small_dense", "nine_dense"])
def test_long_probe_chains(world, table):
    """a table of between one and two slots per key: walks of three and more buckets, counted on the host"""
    w = world
    tab = w[table]
    lay = tab.db.layout()
    assert lay["slots_per_key"] == 1 and lay["n_slots"] > len(tab.keys), lay        # (a full table has no end for a walk)
    reads = [tab.bases[int(tab.off[i]):int(tab.off[i + 1])] for i in range(N_OPT)]
    walks = miss_walks(tab.keys, int(lay["n_slots"]), np.concatenate([features_of(r) for r in reads]))
    print(table, lay, "walks of features that are not in the table:", np.bincount(walks)[:12])
    assert (walks >= 3).any(), "no walk of three buckets"
    ll._check(w, tab, N_OPT, False, ll._device_run(w, tab, N_OPT, False, 2, 2, 0), "%s, %d reads" % (table, N_OPT))
