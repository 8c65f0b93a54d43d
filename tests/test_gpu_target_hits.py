"""mcq_target_hits (include/mcq.h, csrc/mcq_target_hits.hip): per slot target the read's per-target candidate and the hit count of
every window of its range -- what the reference's matches_per_target::insert keeps (src/matches_per_target.h:111-155).  The expected
values come from the oracle alone: OracleDb.target_cands gives (tgt, hits, beg, end) per target of a read, OracleDb.matches the
sorted match list whose entries on that target inside [beg, end] are the windows and counts."""
import importlib

import numpy as np
import pytest
import torch

from golden_util import Fixture
from oracle import dbfile
from oracle import mc_oracle as orc

pytestmark = pytest.mark.gpu

FILL = 0xDEADBEEF
UNUSED = 0xFFFFFFFF


def _eng():
    return importlib.import_module("metacache-mpi_amd.engine")


def expected_of_read(odb, s1, s2, insert):
    """{tgt: (hits, beg, counts[end - beg + 1])} and the target order of target_cands"""
    tc = odb.target_cands(s1, s2, insert)
    m = odb.matches(s1, s2)
    mt = (m >> np.uint64(32)).astype(np.int64); mw = (m & np.uint64(0xFFFFFFFF)).astype(np.int64)
    out, order = {}, []
    for tgt, hits, beg, end in tc.astype(np.int64):
        sel = mw[(mt == tgt) & (mw >= beg) & (mw <= end)]
        cnt = np.bincount(sel - beg, minlength=end - beg + 1).astype(np.uint32)
        assert cnt.sum() == hits and cnt[0] > 0 and cnt[-1] > 0      # (the oracle's own two functions agree)
        out[int(tgt)] = (int(hits), int(beg), cnt)
        order.append(int(tgt))
    return out, order


def make_slots(orders, n_slots, n_targets):
    """per query: the first targets of target_cands, one target the read does not hit and one unused slot (n_slots 1: one of the
    three in turn; n_slots 2: a hit target and one of the other two in turn)"""
    slots = np.full((len(orders), n_slots), UNUSED, np.uint32)
    for q, order in enumerate(orders):
        miss = next(t for t in range(n_targets) if t not in order) if len(order) < n_targets else UNUSED
        if n_slots == 1:
            slots[q, 0] = (order[0] if order else miss) if q % 3 == 0 else (miss if q % 3 == 1 else UNUSED)
        elif n_slots == 2:
            slots[q, 0] = order[0] if order else miss
            slots[q, 1] = miss if q % 2 else UNUSED
        else:
            hit = order[:n_slots - 2]
            slots[q, :len(hit)] = hit
            slots[q, n_slots - 2] = miss                  # (behind unused slots when the read hits few targets)
    return slots


def check(ranges, counts, status, slots, exps, ctx):
    assert not status.any(), (ctx, np.nonzero(status)[0][:5], status[status != 0][:5])
    for q, (exp, _) in enumerate(exps):
        for s, tgt in enumerate(slots[q].tolist()):
            r = ranges[q, s].tolist()
            assert r[0] == tgt, (ctx, q, s, r)
            if tgt in exp:
                hits, beg, cnt = exp[tgt]
                assert r[1:] == [hits, beg, len(cnt)], (ctx, q, s, r, exp[tgt])
                assert np.array_equal(counts[q, s, :len(cnt)], cnt), (ctx, q, s, counts[q, s, :len(cnt)], cnt)
                assert (counts[q, s, len(cnt):] == FILL).all(), (ctx, q, s)
            else:                                         # a target the read does not hit, or an unused slot
                assert r[1:] == [0, 0, 0], (ctx, q, s, r)
                assert (counts[q, s] == FILL).all(), (ctx, q, s)


# ---- the golden fixtures ----------------------------------------------------------------------------------------------
_fx_cache = {}


def fixture_world(tag):
    """the fixture's table, reads and, per (paired), the oracle's answers -- computed once, shared by every case"""
    if tag not in _fx_cache:
        fx = Fixture(tag, 2)
        keys, off, locs = dbfile.union_shards(fx.shards)
        p = fx.params
        t2t = fx.tax.target_keys(fx.n_targets, 0)
        kw = dict(k=p["qk"], winlen=p["qwinlen"], winstride=p["qwinstride"], tgt_winstride=p["winstride"])
        odb = orc.OracleDb(keys, off, locs, t2t, s=p["qs"], **kw)
        seqs = fx.interleaved()
        rb, ro = orc.pack_reads(seqs)
        exps = {}
        for paired, insert in ((True, 400), (False, 0)):
            qs = [(seqs[2 * i], seqs[2 * i + 1]) for i in range(len(seqs) // 2)] if paired else [(s, "") for s in seqs]
            exps[paired] = ([expected_of_read(odb, a, b, insert) for a, b in qs], insert)
        assert all(sum(len(o) > 0 for _, o in ex) >= len(ex) // 2 for ex, _ in exps.values())     # half of the reads or more hit a target
        _fx_cache[tag] = (fx, keys, off, locs, t2t, dict(sketch_size=p["qs"], **kw), rb, ro, exps)
    return _fx_cache[tag]


@pytest.mark.parametrize("locflags", ["fields32", "fields64", "gw"])
@pytest.mark.parametrize("tag", ["mini", "tie", "overpop"])
def test_fixtures_in_every_location_form(tag, locflags):
    eng = _eng()
    fx, keys, off, locs, t2t, kw, rb, ro, exps = fixture_world(tag)
    lf = {"fields32": 0, "fields64": eng.MCQ_DB_LOCS_64, "gw": eng.MCQ_DB_LOCS_GW}[locflags]
    want_form = {"fields32": eng.MCQ_LOC_FIELDS32, "fields64": eng.MCQ_LOC_FIELDS64, "gw": eng.MCQ_LOC_GLOBAL_WINDOW}[locflags]
    packed_bases = eng.pack_bases_host(rb)
    for layout in (eng.MCQ_DB_BUCKETS_64, eng.MCQ_DB_SLOTS_16):
        db = eng.Database(keys, off, locs, t2t, flags=lf | layout, **kw)
        lay = db.layout()
        assert lay["loc_format"] == want_form and lay["bucket_bytes"] == (64 if layout == eng.MCQ_DB_BUCKETS_64 else 16)
        ws = eng.Workspace(db, len(ro) - 1, len(rb) + 64)
        for paired in (True, False):
            ex, insert = exps[paired]
            for n_slots in (1, 2, 16):
                slots = make_slots([o for _, o in ex], n_slots, fx.n_targets)
                for packed in (False, True):
                    if packed and (n_slots == 2 or layout == eng.MCQ_DB_SLOTS_16):
                        continue                          # (the batch's form does not meet the slot logic or the layout: two cases suffice)
                    r, c, st = ws.target_hits_host(packed_bases if packed else rb, ro, paired, slots, insert_size_max=insert,
                                                   packed=packed, fill=FILL)
                    check(r, c, st, slots, ex, (tag, locflags, layout, paired, n_slots, packed))


@pytest.mark.parametrize("paired", [False, True])
def test_batch_given_as_ranges(paired):
    """MCQ_BATCH_RANGES: (begin, end) byte ranges into a buffer in which the reads lie in another order than the queries, with
    other text between them and in front of the first"""
    eng = _eng()
    fx, keys, off, locs, t2t, kw, rb, ro, exps = fixture_world("mini")
    db = eng.Database(keys, off, locs, t2t, **kw)
    ex, insert = exps[paired]
    n = len(ro) - 1
    rng = np.random.default_rng(11)
    order = rng.permutation(n)
    buf, rg = bytearray(b"@header of nothing\n"), np.zeros(2 * n, np.uint64)
    for i in order.tolist():
        rg[2 * i] = len(buf)
        buf += rb[int(ro[i]):int(ro[i + 1])]
        rg[2 * i + 1] = len(buf)
        buf += b"\n+\nIIII\n@gap" * int(rng.integers(0, 3))
    ws = eng.Workspace(db, n, len(buf) + 64)
    slots = make_slots([o for _, o in ex], 16, fx.n_targets)
    r, c, st = ws.target_hits_host(bytes(buf), rg, paired, slots, insert_size_max=insert, fill=FILL, ranges=True)
    check(r, c, st, slots, ex, ("ranges", paired))


# ---- boundary lengths and non-default geometries on a small synthetic table --------------------------------------------
@pytest.mark.parametrize("k,s,W,S", [(12, 8, 64, 53), (16, 16, 128, 64)])
def test_boundary_lengths(k, s, W, S):
    eng = _eng()
    dbbuild = importlib.import_module("dbbuild_torch")
    synth = importlib.import_module("metacache-mpi_amd.synth")
    dev = torch.device("cuda", 0)
    gb, goff, species = synth.make_genomes(4, 5, 30_000, 60_000, 0.03, seed=17, device=dev)
    keys, off, locs, _ = dbbuild.build_table(gb, goff, emulate_ranks=2, k=k, s=s, winlen=W, winstride=S)
    n_targets = goff.numel() - 1
    t2t = (torch.arange(n_targets, device=dev) | 0x80000000)
    hk, ho, hl = (x.cpu().numpy() for x in (keys, off, locs))
    odb = orc.OracleDb(hk.astype(np.uint32), ho.astype(np.uint64), hl.astype(np.uint64), t2t.cpu().numpy().astype(np.uint32),
                       k=k, s=s, winlen=W, winstride=S, tgt_winstride=S)
    over64 = W + S * (64 // s - 1) + 1                    # one window more than 64 features' worth
    lengths = [k - 1, k, 127, 128, 129, 240, 241, 242, over64, W, W + 1, W + S, W + S + 1]
    host = gb.cpu().numpy(); offs = goff.cpu().numpy()
    rng = np.random.default_rng(5)
    seqs = []
    for rep in range(4):
        for L in lengths:
            t = int(rng.integers(0, n_targets))
            a = int(rng.integers(offs[t], offs[t + 1] - L))
            seqs.append(host[a:a + L].tobytes())
    rb, ro = orc.pack_reads(seqs)
    for lf in (0, eng.MCQ_DB_LOCS_64, eng.MCQ_DB_LOCS_GW):
        db = dbbuild.make_database(keys, off, locs, t2t, k=k, s=s, winlen=W, winstride=S, tgt_winstride=S, flags=lf)
        ws = eng.Workspace(db, len(seqs), len(rb) + 64)
        for paired, insert in ((False, 0), (True, 300)):
            qs = [(seqs[2 * i], seqs[2 * i + 1]) for i in range(len(seqs) // 2)] if paired else [(x, b"") for x in seqs]
            ex = [expected_of_read(odb, a, b, insert) for a, b in qs]
            assert sum(len(o) > 0 for _, o in ex) > len(ex) // 2
            slots = make_slots([o for _, o in ex], 5, n_targets)
            r, c, st = ws.target_hits_host(rb, ro, paired, slots, insert_size_max=insert, fill=FILL)
            check(r, c, st, slots, ex, (k, s, W, S, lf, paired))


# ---- long reads ---------------------------------------------------------------------------------------------------------
def test_long_reads_against_two_strains():
    eng = _eng()
    dbbuild = importlib.import_module("dbbuild_torch")
    synth = importlib.import_module("metacache-mpi_amd.synth")
    dev = torch.device("cuda", 0)
    gb, goff, species = synth.make_genomes(1, 2, 60_000, 80_000, 0.01, seed=23, device=dev)
    keys, off, locs, _ = dbbuild.build_table(gb, goff, emulate_ranks=1)
    t2t = (torch.arange(2, device=dev) | 0x80000000)
    db = dbbuild.make_database(keys, off, locs, t2t)
    odb = orc.OracleDb(keys.cpu().numpy().astype(np.uint32), off.cpu().numpy().astype(np.uint64), locs.cpu().numpy().astype(np.uint64),
                       t2t.cpu().numpy().astype(np.uint32))
    reads, roff, _ = synth.sample_long_reads(gb, goff, 4, 20000, 0.0, seed=1, min_len=15000, max_len=25000)
    rb = reads.cpu().numpy().tobytes(); ro = roff.cpu().numpy().astype(np.uint64)
    ex = [expected_of_read(odb, rb[int(ro[i]):int(ro[i + 1])], b"", 0) for i in range(4)]
    assert all(len(o) == 2 for _, o in ex) and min(len(e[t][2]) for e, _ in ex for t in e) > 100      # wide ranges on both strains
    slots = np.array([[o[1], UNUSED, o[0]] for _, o in ex], np.uint32)
    ws = eng.Workspace(db, 4, len(rb) + 64)
    r, c, st = ws.target_hits_host(rb, ro, False, slots, fill=FILL)
    check(r, c, st, slots, ex, "long")


# ---- capacity: reported, never a fault and never a wrong answer --------------------------------------------------------------
def test_capacity_is_reported_per_query():
    eng = _eng()
    dbbuild = importlib.import_module("dbbuild_torch")
    synth = importlib.import_module("metacache-mpi_amd.synth")
    dev = torch.device("cuda", 0)
    gb, goff, species = synth.make_genomes(4, 4, 30_000, 40_000, 0.03, seed=31, device=dev)       # 16 targets
    keys, off, locs, _ = dbbuild.build_table(gb, goff, emulate_ranks=1)
    t2t = (torch.arange(16, device=dev) | 0x80000000)
    db = dbbuild.make_database(keys, off, locs, t2t)
    odb = orc.OracleDb(keys.cpu().numpy().astype(np.uint32), off.cpu().numpy().astype(np.uint64), locs.cpu().numpy().astype(np.uint64),
                       t2t.cpu().numpy().astype(np.uint32))
    host = gb.cpu().numpy(); offs = goff.cpu().numpy()
    big = b"".join(host[offs[t]:offs[t] + 10_000].tobytes() for t in range(16))                 # 160 kb over all 16 targets
    small = [host[offs[3] + 500:offs[3] + 650].tobytes(), host[offs[9] + 7000:offs[9] + 7150].tobytes()]
    m = odb.matches(big)
    assert len(np.unique(m)) > eng.MCQ_TARGET_HITS_MAX_KEYS                                      # the read is what the case needs
    seqs = [small[0], big, small[1]]
    rb, ro = orc.pack_reads(seqs)
    ex = [expected_of_read(odb, s, b"", 0) for s in seqs]
    slots = np.tile(np.arange(16, dtype=np.uint32), (3, 1))
    ws = eng.Workspace(db, 3, len(rb) + 64)
    cap = ws.target_hits_range_cap(len(big))
    assert cap == 2 + len(big) // 113
    r, c, st = ws.target_hits_host(rb, ro, False, slots, range_cap=cap, fill=FILL, sync=False)
    assert st.tolist() == [0, eng.MCQ_TARGET_HITS_KEYS, 0]
    assert (r[1, :, 3] == 0).all() and (r[1, :, 1] == 0).all() and r[1, :, 0].tolist() == list(range(16)) and (c[1] == FILL).all()
    keep = [0, 2]
    check(r[keep], c[keep], st[keep], slots[keep], [ex[0], ex[2]], "neighbours of the large read")
    with pytest.raises(eng.McqError) as e:
        ws.sync()
    assert e.value.code == eng.MCQ_E_CAPACITY

    # a range_cap one short of what the longest query needs
    seqs = [small[0], host[offs[5] + 100:offs[5] + 400].tobytes(), small[1]]
    rb, ro = orc.pack_reads(seqs)
    ex = [expected_of_read(odb, s, b"", 0) for s in seqs]
    ws = eng.Workspace(db, 3, len(rb) + 64)
    cap = ws.target_hits_range_cap(300)
    assert cap == 4 and ws.target_hits_range_cap(150) == 3 and ws.target_hits_range_cap(150, 400) == 5
    r, c, st = ws.target_hits_host(rb, ro, False, slots, range_cap=cap, fill=FILL)               # the helper's value: no error
    check(r, c, st, slots, ex, "cap")
    r, c, st = ws.target_hits_host(rb, ro, False, slots, range_cap=cap - 1, fill=FILL, sync=False)
    assert st.tolist() == [0, eng.MCQ_TARGET_HITS_RANGE, 0]
    assert (r[1, :, 1:] == 0).all() and (c[1] == FILL).all()
    check(r[keep], c[keep], st[keep], slots[keep], [ex[0], ex[2]], "neighbours of the wide read")
    with pytest.raises(eng.McqError) as e:
        ws.sync()
    assert e.value.code == eng.MCQ_E_CAPACITY


def test_rejected_arguments():
    eng = _eng()
    z = (np.zeros(0, np.uint32), np.zeros(1, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
    db = eng.Database(*z)
    ws = eng.Workspace(db, 4, 64)
    one = torch.zeros(64, dtype=torch.int32, device="cuda")
    for n_slots, cap in ((0, 3), (17, 3), (2, 0)):
        with pytest.raises(eng.McqError) as e:
            ws.target_hits(one.data_ptr(), one.data_ptr(), 1, False, one.data_ptr(), n_slots, cap, one.data_ptr(), one.data_ptr(), one.data_ptr())
        assert e.value.code == eng.MCQ_E_ARG
    # an empty table: every slot answered with no range; a target id the table does not have is no fault
    r, c, st = ws.target_hits_host(b"ACGTACGTACGTACGTACGTACGT", np.array([0, 24], np.uint64), False, np.array([[0, 5]], np.uint32), fill=FILL)
    assert r.tolist() == [[[0, 0, 0, 0], [5, 0, 0, 0]]] and st.tolist() == [0] and (c == FILL).all()


# ---- mcq_target_slots: the slot targets from a batch's device results -------------------------------------------------------
def test_target_slots_from_device_results():
    eng = _eng()
    dev = torch.device("cuda", 0)
    SEQ = 0x80000000
    tax2tgt = np.array([UNUSED, 4, UNUSED, 0, 2], np.uint32)          # taxon index -> target
    #          tax          hits
    cands = np.array([[[SEQ | 1, 9, 0, 0], [SEQ | 3, 5, 0, 0], [SEQ | 4, 2, 0, 0]],        # third below hits_min
                      [[2, 9, 0, 0], [SEQ | 4, 8, 0, 0], [SEQ | 3, 8, 0, 0]],               # first above sequence level
                      [[SEQ | 1, 9, 0, 0], [SEQ | 3, 9, 0, 0], [SEQ | 4, 9, 0, 0]],        # n_cand = 1: the rest is stale
                      [[SEQ | 0, 9, 0, 0], [SEQ | 7, 9, 0, 0], [UNUSED, 9, 0, 0]]], np.uint32)   # no target / beyond the table / none
    ncand = np.array([3, 3, 1, 3], np.uint32)
    dc = torch.from_numpy(cands.view(np.int32)).to(dev); dn = torch.from_numpy(ncand.view(np.int32)).to(dev)
    dt = torch.from_numpy(tax2tgt.view(np.int32)).to(dev)
    for n_slots, want in ((2, [[4, 0], [2, 0], [4, UNUSED], [UNUSED, UNUSED]]), (1, [[4], [2], [4], [UNUSED]]),
                          (4, [[4, 0, UNUSED, UNUSED], [2, 0, UNUSED, UNUSED], [4, UNUSED, UNUSED, UNUSED], [UNUSED] * 4])):
        out = torch.full((4, n_slots), 77, dtype=torch.int32, device=dev)
        eng.target_slots(dc.data_ptr(), dn.data_ptr(), 4, 3, 5, dt.data_ptr(), len(tax2tgt), out.data_ptr(), n_slots,
                         stream=torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
        assert out.cpu().numpy().view(np.uint32).tolist() == want
