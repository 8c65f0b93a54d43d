"""mcq_all_hits_count / mcq_all_hits (include/mcq.h, csrc/mcq_all_hits.hip): a read's sorted match list, run-length compressed.

The expected entries are the RLE (tests/all_hits_ref.py) of OracleDb.matches, the CPU restatement that tests/test_oracle_golden.py
pins to the reference.  The tables are made by mcq_db_create from hand-built arrays: a read's features come from the oracle's
sketch, and each gets a list of a chosen length drawn from a pool of locations of a chosen size, so that both the read's location
count and its number of distinct locations are set, not hoped for.  Workspace.debug_matches, run-length compressed, is a second,
independent GPU path where the batch is a plain host batch."""
import importlib

import numpy as np
import pytest
import torch

import all_hits_ref as ahr
from all_hits_harness import all_hits_guarded
from golden_util import Fixture
from oracle import dbfile
from oracle import mc_oracle as orc

pytestmark = pytest.mark.gpu

# windows per target: one window next to many, so that the width of the window bit field and the global-window prefix both matter
TGT_WINDOWS = np.array([1, 5000, 3, 700, 1, 40000], np.uint32)


def _eng():
    return importlib.import_module("metacache-mpi_amd.engine")


def rand_read(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n).tolist())


def probes_of(seqs, k, s, winlen, stride):
    """the features the kernel probes for a read (pair), window by window: a feature of two windows is probed twice"""
    out = []
    for seq in seqs:
        for b, e in orc.windows(len(seq), winlen, stride):
            out += orc.sketch(seq[b:e], k, s).tolist()
    return out


def location_pool(rng, n):
    """n distinct (tgt << 32) | win, ascending, with the corners of the (target, window) space among them"""
    corners = [(0, 0), (1, 0), (1, 4999), (2, 2), (4, 0), (5, 39999), (5, 0)]
    assert n >= len(corners)
    have = set(corners)
    while len(have) < n:
        t = int(rng.integers(0, len(TGT_WINDOWS)))
        have.add((t, int(rng.integers(0, TGT_WINDOWS[t]))))
    return np.array(sorted((t << 32) | w for t, w in have), np.uint64)


def make_table(reads, T_of, D_of, geom, seed=1):
    """reads: list of reads (tuples of one or two sequences) with pairwise different features; read i gets T_of[i] locations of which
    D_of[i] are distinct.  Returns keys, off, locs of the table."""
    rng = np.random.default_rng(seed)
    lists = {}
    for seqs, T, D in zip(reads, T_of, D_of):
        pr = probes_of(seqs, *geom)
        mult = {}
        for f in pr:
            mult[f] = mult.get(f, 0) + 1
        assert not (set(mult) & set(lists)), "two reads share a feature"
        feats = sorted(mult)
        if T == 0:
            continue
        singles = [f for f in feats if mult[f] == 1]
        assert singles and 1 <= D <= T
        pool = location_pool(rng, max(D, 7))[:D] if D < 7 else location_pool(rng, D)
        # lengths: spread T over the features, the remainder on features that are probed once
        n = len(feats)
        base = T // sum(mult.values())
        lens = {f: base for f in feats}
        rest = T - sum(lens[f] * mult[f] for f in feats)
        i = 0
        while rest > 0:
            lens[singles[i % len(singles)]] += 1
            rest -= 1; i += 1
        assert sum(lens[f] * mult[f] for f in feats) == T and max(lens.values()) <= D
        start = 0
        for f in feats:                                     # consecutive stretches of the pool, wrapping: the union covers it
            idx = (start + np.arange(lens[f])) % D
            lists[f] = np.sort(pool[idx])
            start += lens[f]
        assert n > 0
    keys = np.array(sorted(lists), np.uint32)
    lens = np.array([len(lists[int(f)]) for f in keys], np.uint64)
    off = np.zeros(len(keys) + 1, np.uint64); off[1:] = np.cumsum(lens)
    locs = np.concatenate([lists[int(f)] for f in keys]) if len(keys) else np.zeros(0, np.uint64)
    return keys, off, locs


GEOM = (16, 16, 128, 113)
WALK = 32                      # AH_WALK_MAX of csrc/mcq_all_hits.hip


def world(reads, T_of, D_of, geom=GEOM, seed=1):
    keys, off, locs = make_table(reads, T_of, D_of, geom, seed)
    k, s, W, S = geom
    t2t = (np.arange(len(TGT_WINDOWS)) | 0x80000000).astype(np.uint32)
    odb = orc.OracleDb(keys, off, locs, t2t, k=k, s=s, winlen=W, winstride=S, tgt_winstride=S)
    exp = [ahr.rle(odb.matches(*r)) for r in reads]
    for e, T, D in zip(exp, T_of, D_of):
        assert int(e["hits"].sum()) == T and len(e) == (D if T else 0)      # each such read is asserted to occur
    return keys, off, locs, t2t, exp


def database(eng, w, flags=0, geom=GEOM):
    k, s, W, S = geom
    return eng.Database(w[0], w[1], w[2], w[3], k=k, sketch_size=s, winlen=W, winstride=S, tgt_winstride=S, flags=flags,
                        tgt_windows=TGT_WINDOWS)


def run(eng, db, reads, paired=False, max_locs=0, **kw):
    seqs = [x for r in reads for x in (r if paired else r[:1])]
    rb, ro = orc.pack_reads(seqs)
    ws = eng.Workspace(db, max(1, len(reads)), len(rb) + 64, max_locs)
    return all_hits_guarded(ws, rb, ro, paired, guard=16, **kw), ws, rb, ro


def guards_intact(res):
    g, raw, tot = res["guard"], res["raw"], res["total"]
    return (raw[:3 * g] == res["fill"]).all() and (raw[3 * (g + tot):] == res["fill"]).all()


def segment_untouched(res, q, off=None):
    off = res["loc_off"] if off is None else off
    g = res["guard"]
    return (res["raw"][3 * (g + int(off[q])):3 * (g + int(off[q + 1]))] == res["fill"]).all()


def check(res, exp, ctx):
    assert not res["status"].any(), (ctx, res["status"])
    assert guards_intact(res), ctx
    for q, e in enumerate(exp):
        assert int(res["loc_off"][q + 1] - res["loc_off"][q]) == int(e["hits"].sum()), (ctx, q)
        assert res["n_hits"][q] == len(e), (ctx, q, res["n_hits"][q], len(e))
        assert np.array_equal(res["hits"][q], e), (ctx, q, res["hits"][q][:8], e[:8])


# ---- every bound between code paths --------------------------------------------------------------------------------------------
_bounds = {}


def bounds_world():
    if not _bounds:
        eng = _eng()
        R, Wv = eng.MCQ_ALL_HITS_REG_MAX, eng.MCQ_ALL_HITS_WAVE_MAX
        assert (R, Wv) == (64, 2048)
        rng = np.random.default_rng(7)
        # (T, D): location counts at every bound of the kernel, distinct counts at a chunk of the run-length pass (64 per wave, 256
        # per workgroup) and at the extremes (all equal, all distinct where the lists allow it)
        cases = [(1, 1), (2, 1), (2, 2), (R - 1, R - 1), (R, R), (R + 1, R + 1), (30, 1), (R + 1, 63), (R + 1, 64), (200, 65), (300, 128),
                 (Wv - 1, Wv // 2), (Wv, 255), (Wv, 256), (Wv, 257), (Wv + 1, 256), (Wv + 1, 257), (Wv + 1, 150), (Wv + 2, 1100),
                 (2 * Wv + 5, 513), (3000, 255)]
        reads = [(rand_read(rng, 150),) for _ in cases]
        # ... and the bound inside the gather (AH_WALK_MAX of csrc/mcq_all_hits.hip, restated: a list of up to 32 words is copied
        # by its lane, a longer one by the whole wave): every list of a read 32 words, every list 33, and both kinds in one read
        for per, extra in ((WALK, 0), (WALK + 1, 0), (WALK, 5)):
            r = (rand_read(rng, 150),)
            n = len(probes_of(r, *GEOM))
            assert n == len(set(probes_of(r, *GEOM)))
            reads.append(r); cases.append((per * n + extra, 200))
        reads, cases = reads[:-5] + reads[-3:] + reads[-5:-3], cases[:-5] + cases[-3:] + cases[-5:-3]      # (the two largest stay last)
        w = world(reads, [c[0] for c in cases], [c[1] for c in cases])
        lens = np.diff(w[1].astype(np.int64))
        assert (lens == WALK).sum() >= 30 and (lens == WALK + 1).sum() >= 30      # lists at the bound occur
        _bounds["w"] = (reads, cases, w)
    return _bounds["w"]


@pytest.mark.parametrize("layout", ["buckets64", "slots16"])
@pytest.mark.parametrize("locform", ["fields32", "fields64", "gw"])
def test_every_bound_in_every_form(locform, layout):
    eng = _eng()
    reads, cases, w = bounds_world()
    lf = {"fields32": 0, "fields64": eng.MCQ_DB_LOCS_64, "gw": eng.MCQ_DB_LOCS_GW}[locform]
    lay = {"buckets64": eng.MCQ_DB_BUCKETS_64, "slots16": eng.MCQ_DB_SLOTS_16}[layout]
    db = database(eng, w, lf | lay)
    got = db.layout()
    assert got["loc_format"] == {"fields32": eng.MCQ_LOC_FIELDS32, "fields64": eng.MCQ_LOC_FIELDS64, "gw": eng.MCQ_LOC_GLOBAL_WINDOW}[locform]
    assert got["bucket_bytes"] == (64 if layout == "buckets64" else 16)
    res, ws, rb, ro = run(eng, db, reads)
    check(res, w[4], (locform, layout))


def test_batch_forms_give_the_same_entries():
    """ASCII against packed, offsets against ranges, single against paired (a pair whose second mate is empty is its first mate)"""
    eng = _eng()
    reads, cases, w = bounds_world()
    db = database(eng, w)
    res, ws, rb, ro = run(eng, db, reads)
    check(res, w[4], "plain")
    packed = all_hits_guarded(ws, eng.pack_bases_host(rb), ro, False, packed=True, guard=16)
    check(packed, w[4], "packed")
    rng = np.random.default_rng(3)
    buf, rg = bytearray(b"@in front\n"), np.zeros(2 * len(reads), np.uint64)
    for i in rng.permutation(len(reads)).tolist():
        rg[2 * i] = len(buf); buf += reads[i][0]; rg[2 * i + 1] = len(buf)
        buf += b"\n+\nII\n@x" * int(rng.integers(0, 3))
    ws2 = eng.Workspace(db, len(reads), len(buf) + 64)
    check(all_hits_guarded(ws2, bytes(buf), rg, False, ranges=True, guard=16), w[4], "ranges")
    pairs = [(r[0], b"") for r in reads]
    res_p, _, _, _ = run(eng, db, pairs, paired=True)
    check(res_p, w[4], "paired with an empty second mate")
    swapped = [(b"", r[0]) for r in reads]
    res_s, _, _, _ = run(eng, db, swapped, paired=True)
    check(res_s, w[4], "paired with an empty first mate")


def test_second_gpu_path_agrees():
    eng = _eng()
    reads, cases, w = bounds_world()
    db = database(eng, w)
    rb, ro = orc.pack_reads([r[0] for r in reads])
    ws = eng.Workspace(db, len(reads), len(rb) + 64)
    moff, m = ws.debug_matches(rb, ro, False)
    for q, e in enumerate(w[4]):
        assert np.array_equal(ahr.rle(m[int(moff[q]):int(moff[q + 1])]), e), q


# ---- small and empty reads -------------------------------------------------------------------------------------------------------
def test_small_reads_and_no_queries():
    eng = _eng()
    rng = np.random.default_rng(11)
    hit1, hit2, mate = rand_read(rng, 150), rand_read(rng, 100), rand_read(rng, 140)
    # read 0: one location; read 1: empty; read 2: shorter than k; read 3: no feature in the table; read 4: a pair with one empty
    # mate; read 5: a real pair
    pairs = [(hit1, b""), (b"", b""), (b"ACGTACGTAC", b""), (rand_read(rng, 150), b""), (b"", hit2), (mate, rand_read(rng, 90))]
    T = [1, 0, 0, 0, 40, 77]
    D = [1, 0, 0, 0, 40, 30]
    w = world(pairs, T, D)
    db = database(eng, w)
    res, ws, rb, ro = run(eng, db, pairs, paired=True)
    check(res, w[4], "small")
    assert res["n_hits"].tolist() == [1, 0, 0, 0, 40, 30]
    singles = [(a,) for a, b in pairs] + [(b,) for a, b in pairs]
    exp = [ahr.rle(orc.OracleDb(w[0], w[1], w[2], w[3], tgt_winstride=113).matches(s[0])) for s in singles]
    res1, _, _, _ = run(eng, db, singles)
    check(res1, exp, "mates alone")
    # no queries at all: loc_off[0] = 0, nothing else is written
    none = all_hits_guarded(ws, b"", np.zeros(1, np.uint64), False, guard=16)
    assert none["loc_off"].tolist() == [0] and guards_intact(none) and len(none["hits"]) == 0


def test_count_beyond_eight_bits():
    """one (target, window) in the list of every feature of every window of a pair of long mates"""
    eng = _eng()
    rng = np.random.default_rng(13)
    pair = (rand_read(rng, 1300), rand_read(rng, 1400))
    pr = probes_of(pair, *GEOM)
    assert len(pr) > 300
    X = (5 << 32) | 39999
    feats = sorted(set(pr))
    keys = np.array(feats, np.uint32)
    lists = [np.array(sorted({X, (1 << 32) | (i % 5000)}), np.uint64) for i in range(len(feats))]
    off = np.zeros(len(keys) + 1, np.uint64); off[1:] = np.cumsum([len(l) for l in lists])
    w = (keys, off, np.concatenate(lists), (np.arange(len(TGT_WINDOWS)) | 0x80000000).astype(np.uint32))
    exp = [ahr.rle(orc.OracleDb(*w, tgt_winstride=113).matches(*pair))]
    assert exp[0][-1].tolist() == (5, 39999, len(pr)) and len(pr) > 255
    for lf in (0, eng.MCQ_DB_LOCS_64, eng.MCQ_DB_LOCS_GW):
        res, _, _, _ = run(eng, database(eng, w, lf), [pair], paired=True)
        check(res, exp, ("count", lf))


def test_long_read():
    """an ONT-like read of 20 kb on a table that gives it a few thousand locations: the workgroup tier, many windows per wave"""
    eng = _eng()
    rng = np.random.default_rng(17)
    reads = [(rand_read(rng, 20000),), (rand_read(rng, 150),)]
    w = world(reads, [7000, 30], [2500, 30])
    for lf in (0, eng.MCQ_DB_LOCS_64):
        res, _, _, _ = run(eng, database(eng, w, lf), reads)
        check(res, w[4], ("long", lf))


def test_other_geometry():
    eng = _eng()
    geom = (12, 8, 64, 53)
    rng = np.random.default_rng(19)
    reads = [(rand_read(rng, L),) for L in (64, 65, 117, 118, 300, 1000, 11, 12)]
    T = [5, 9, 16, 70, 500, 2100, 0, 1]
    D = [5, 4, 16, 64, 333, 1999, 0, 1]
    w = world(reads, T, D, geom)
    for lf in (0, eng.MCQ_DB_LOCS_GW):
        res, _, _, _ = run(eng, database(eng, w, lf, geom), reads)
        check(res, w[4], ("geometry", lf))


# ---- capacities and safety -----------------------------------------------------------------------------------------------------
def test_more_locations_than_the_workspace_takes():
    eng = _eng()
    rng = np.random.default_rng(23)
    reads = [(rand_read(rng, 150),) for _ in range(4)]
    T, D = [100, 4097, 4096, 3], [50, 300, 4000, 3]
    w = world(reads, T, D)
    for lf in (0, eng.MCQ_DB_LOCS_64):
        res, _, _, _ = run(eng, database(eng, w, lf), reads, max_locs=4096)
        assert res["status"].tolist() == [0, eng.MCQ_ALL_HITS_LOCS, 0, 0] and res["n_hits"].tolist() == [50, 0, 4000, 3]
        assert np.diff(res["loc_off"].astype(np.int64)).tolist() == T
        assert segment_untouched(res, 1) and guards_intact(res)
        for q in (0, 2, 3):
            assert np.array_equal(res["hits"][q], w[4][q]), q


def test_cap_and_shifted_offsets():
    eng = _eng()
    reads, cases, w = bounds_world()
    reads = reads + [(b"",)]                                  # an empty query behind the last one that has locations
    exp = w[4] + [ahr.rle(np.zeros(0, np.uint64))]
    db = database(eng, w)
    res, ws, rb, ro = run(eng, db, reads)
    check(res, exp, "with an empty read at the end")
    total = int(res["loc_off"][-1])
    # cap one below the total: exactly the last query that has locations is flagged (a workgroup-tier one), the others are answered
    short = all_hits_guarded(ws, rb, ro, False, guard=16, cap=total - 1)
    last = len(cases) - 1
    assert short["status"].tolist() == [0] * last + [eng.MCQ_ALL_HITS_SEGMENT, 0] and short["n_hits"][last] == 0
    assert segment_untouched(short, last) and guards_intact(short)
    for q in range(last):
        assert np.array_equal(short["hits"][q], exp[q]), q
    # the same with a wave-tier query at the end
    order = list(range(len(cases)))
    order.remove(4); order.append(4)
    reads2 = [reads[i] for i in order]
    res2, ws2, rb2, ro2 = run(eng, db, reads2)
    short2 = all_hits_guarded(ws2, rb2, ro2, False, guard=16, cap=int(res2["loc_off"][-1]) - 1)
    assert short2["status"].tolist() == [0] * last + [eng.MCQ_ALL_HITS_SEGMENT] and segment_untouched(short2, last) and guards_intact(short2)
    # offsets shifted behind one query: its segment is one entry too long -- that query alone is flagged, the others are answered
    # at their shifted places.  Once for a query of each tier.
    for bad in (5, 12, len(cases) - 2):
        off = res["loc_off"].copy()
        off[bad + 1:] += np.uint64(1)
        sh = all_hits_guarded(ws, rb, ro, False, guard=16, loc_off=off, cap=int(off[-1]))
        want = [0] * len(reads); want[bad] = eng.MCQ_ALL_HITS_SEGMENT
        assert sh["status"].tolist() == want, bad
        assert segment_untouched(sh, bad, off) and guards_intact(sh) and sh["n_hits"][bad] == 0
        for q in range(len(reads)):
            if q != bad:
                assert np.array_equal(sh["hits"][q], exp[q]), (bad, q)
    # offsets that decrease
    off = res["loc_off"].copy()
    off[3] = off[2] - np.uint64(1)
    dec = all_hits_guarded(ws, rb, ro, False, guard=16, loc_off=off, cap=total)
    assert dec["status"][2] == eng.MCQ_ALL_HITS_SEGMENT and dec["status"][3] == eng.MCQ_ALL_HITS_SEGMENT and guards_intact(dec)
    assert not dec["status"][4:].any() and not dec["status"][:2].any()


def test_a_host_batch_is_refused():
    eng = _eng()
    z = (np.zeros(0, np.uint32), np.zeros(1, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
    db = eng.Database(*z)
    ws = eng.Workspace(db, 4, 64)
    one = torch.zeros(64, dtype=torch.int64, device="cuda")
    p = one.data_ptr()
    import ctypes as C
    host_batch = eng.Batch(1, p, p, 0, 0, 0)                      # no MCQ_DEVICE_PTRS
    assert eng.lib().mcq_all_hits_count(db.h, ws.h, C.byref(host_batch), p, None) == eng.MCQ_E_ARG
    assert eng.lib().mcq_all_hits(db.h, ws.h, C.byref(host_batch), p, p, 1, p, p, None) == eng.MCQ_E_ARG
    assert b"MCQ_DEVICE_PTRS" in eng.lib().mcq_last_error()
    # an empty table: every query has no hit
    res = all_hits_guarded(ws, b"ACGTACGTACGTACGTACGTACGT", np.array([0, 24], np.uint64), False, guard=4)
    assert res["loc_off"].tolist() == [0, 0] and res["n_hits"].tolist() == [0] and res["status"].tolist() == [0] and guards_intact(res)


# ---- the golden fixtures -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,P", [("mini", 2), ("mini", 4), ("mini", 8), ("tie", 2), ("tie", 4)])
def test_fixtures_on_the_union_table(tag, P):
    eng = _eng()
    fx = Fixture(tag, P)
    keys, off, locs = dbfile.union_shards(fx.shards)
    p = fx.params
    t2t = fx.tax.target_keys(fx.n_targets, 0)
    kw = dict(k=p["qk"], winlen=p["qwinlen"], winstride=p["qwinstride"], tgt_winstride=p["winstride"])
    odb = orc.OracleDb(keys, off, locs, t2t, s=p["qs"], **kw)
    seqs = fx.interleaved()
    rb, ro = orc.pack_reads(seqs)
    db = eng.Database(keys, off, locs, t2t, sketch_size=p["qs"], **kw)
    ws = eng.Workspace(db, len(seqs), len(rb) + 64)
    exp = [ahr.rle(odb.matches(a, b)) for a, b in zip(fx.r1, fx.r2)]
    assert sum(len(e) > 0 for e in exp) > len(exp) // 2
    check(all_hits_guarded(ws, rb, ro, True, guard=16), exp, (tag, P, "paired"))
    exp1 = [ahr.rle(odb.matches(s)) for s in seqs]
    check(all_hits_guarded(ws, rb, ro, False, guard=16), exp1, (tag, P, "single"))
    hits, status = ws.all_hits_host(rb, ro, True)                 # the library's own convenience form
    assert not status.any() and all(np.array_equal(h, e) for h, e in zip(hits, exp))
    moff, m = ws.debug_matches(rb, ro, True)
    for q, e in enumerate(exp):
        assert np.array_equal(ahr.rle(m[int(moff[q]):int(moff[q + 1])]), e), q
