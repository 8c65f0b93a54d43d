"""The lean first wave stage (MCQ_FORCE_LEAN_WAVE) against the full one (MCQ_FORCE_FULL_WAVE), the automatic choice between
them over consecutive batches of one workspace, and the CPU oracle: candidate counts and live candidate slots bit for bit, and
the same mcq_stats on both routes.

One small table (150-300 kb genomes): 6 species x 4 strains and a seventh species of 44 strains -- a read of that one
gathers more than 256 locations (16 features x up to 44 strains), which the lean stage hands to the second wave stage; the
table is loaded in both layouts and in the global-window location form.  One batch of 4 096 queries mixes what the first stage can meet: 150 bp reads, reads shorter than k, reads of exactly
one window, reads with runs of N, reads of 450-900 bp (more than 64 features: queued by their geometry), random reads
without hits, and the long-list reads.  Single-end the batch is 4 096 reads; paired, its 4 096 pairs are those reads and
4 096 more of the same mix as the mates."""
import importlib

import numpy as np
import pytest
import torch

from oracle import mc_oracle as orc

pytestmark = pytest.mark.gpu

NQ = 4096


def _genomes(synth, dev):
    """6 species x 4 strains, and a seventh species of 44 strains (targets 24..67)"""
    parts = [synth.make_genomes(6, 4, 150_000, 300_000, 0.02, seed=31, device=dev),
             synth.make_genomes(1, 44, 150_000, 300_000, 0.03, seed=32, device=dev)]
    gb = torch.cat([p[0] for p in parts])
    lens = torch.cat([p[1][1:] - p[1][:-1] for p in parts])
    goff = torch.zeros(lens.numel() + 1, dtype=torch.int64, device=dev)
    goff[1:] = torch.cumsum(lens, 0)
    species = torch.cat([parts[0][2], parts[1][2] + 6])
    return gb, goff, species


def _mixed_reads(synth, gb, goff, n, seed, long_from):
    """n reads as (bytes, offsets): the mix of the module docstring.  long_from: first target of the many-strain species (its
    reads gather the long lists)"""
    dev = gb.device
    rng = np.random.default_rng(seed)
    kinds = rng.choice(7, size=n, p=[0.52, 0.04, 0.08, 0.08, 0.08, 0.08, 0.12])
    src, soff, _ = synth.sample_reads(gb, goff, n, 900, 0.005, 0.0, seed=seed)              # a 900 bp stretch per read
    src = src.cpu().numpy().reshape(n, 900)
    sub_off = goff[long_from:] - goff[long_from]          # kind 6: from the many-strain species
    lsrc, _, _ = synth.sample_reads(gb[int(goff[long_from]):], sub_off, n, 150, 0.002, 0.0, seed=seed + 1)
    lsrc = lsrc.cpu().numpy().reshape(n, 150)
    out = []
    for i, kd in enumerate(kinds):
        if kd == 0: r = src[i, :150]
        elif kd == 1: r = src[i, :int(rng.integers(1, 16))]                   # shorter than k = 16
        elif kd == 2: r = src[i, :int(rng.choice([16, 100, 127, 128]))]         # exactly one window (winlen 128)
        elif kd == 3:                                                           # runs of N
            r = src[i, :150].copy()
            for _ in range(int(rng.integers(1, 4))):
                a = int(rng.integers(0, 150)); r[a:a + int(rng.integers(1, 40))] = 78
        elif kd == 4: r = src[i, :int(rng.integers(450, 901))]                  # 5-8 windows: 80-128 features
        elif kd == 5: r = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=150)]       # no hits
        else: r = lsrc[i]
        out.append(np.ascontiguousarray(r, dtype=np.uint8))
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in out])
    return np.concatenate(out).tobytes(), off


@pytest.fixture(scope="module")
def world():
    """the table (host arrays), the oracle, the reads and the oracle's answers per (paired, P, M) -- computed once"""
    eng = importlib.import_module("metacache-mpi_amd.engine")
    dbbuild = importlib.import_module("dbbuild_torch")
    synth = importlib.import_module("metacache-mpi_amd.synth")
    dev = torch.device("cuda", 0)
    gb, goff, species = _genomes(synth, dev)
    keys, off, locs, _ = dbbuild.build_table(gb, goff, emulate_ranks=2)
    odb = orc.OracleDb(keys.cpu().numpy().astype(np.uint32), off.cpu().numpy().astype(np.uint64),
                       locs.cpu().numpy().astype(np.uint64), species.cpu().numpy().astype(np.uint32))
    rb, ro = _mixed_reads(synth, gb, goff, 2 * NQ, seed=7, long_from=24)
    single = (rb[:int(ro[NQ])], ro[:NQ + 1].copy())
    # a calm batch for the automatic choice: 150 bp reads of the 4-strain species only (short lists, few distinct locations)
    cr, co, _ = synth.sample_reads(gb[:int(goff[24])], goff[:25], 2 * NQ, 150, 0.005, 0.001, seed=9)
    cb, co = cr.cpu().numpy().tobytes(), co.cpu().numpy().astype(np.uint64)
    calm = {False: (cb[:int(co[NQ])], co[:NQ + 1].copy()), True: (cb, co)}
    want, want_calm = {}, {}
    for paired in (False, True):
        b, o = (rb, ro) if paired else single
        for P, M in ((2, 2), (8, 4)):
            want[paired, P, M] = odb.query(b, o, paired, max_cand=M, emulate_ranks=P, insert_size_max=0, threads=8)
            want_calm[paired, P, M] = odb.query(*calm[paired], paired, max_cand=M, emulate_ranks=P, insert_size_max=0, threads=8)
    return eng, dbbuild, (keys, off, locs, species), single, (rb, ro), want, calm, want_calm


def _same(cands, ncand, oc, on, what):
    assert np.array_equal(ncand, on), (what, "n_cand differs at", np.nonzero(ncand != on)[0][:5])
    mask = np.arange(cands.shape[1])[None, :] < on[:, None]
    assert np.array_equal(cands[mask], oc[mask]), (what, "candidate slots differ")


AUTO = True          # the automatic choice between the two forms is on (MCQ_LEAN_AUTO in csrc/mcq_engine.hip)
STATS = ("n_queries", "n_features", "n_hit_features", "n_locations", "n_cands", "n_overflow")


@pytest.mark.parametrize("dbflags", ["slots16", "buckets64", "gw"])
@pytest.mark.parametrize("paired", [False, True])
def test_lean_equals_full_equals_oracle(world, dbflags, paired):
    eng, dbbuild, (keys, off, locs, species), single, both, want, calm, want_calm = world
    fl = {"slots16": eng.MCQ_DB_SLOTS_16, "buckets64": eng.MCQ_DB_BUCKETS_64, "gw": eng.MCQ_DB_LOCS_GW}[dbflags]
    db = dbbuild.make_database(keys, off, locs, species, flags=fl)
    if dbflags == "gw":
        assert db.layout()["loc_format"] == eng.MCQ_LOC_GLOBAL_WINDOW
    rb, ro = both if paired else single
    for P, M in ((2, 2), (8, 4)):
        oc, on = want[paired, P, M]
        ws = eng.Workspace(db, NQ, len(rb))
        res = {}
        for name, qf in (("full", eng.MCQ_FORCE_FULL_WAVE), ("lean", eng.MCQ_FORCE_LEAN_WAVE)):
            c, n = ws.query_host(rb, ro, paired, max_cand=M, emulate_ranks=P, flags=qf)
            res[name] = (c, n, ws.sync())
            _same(c, n, oc, on, (name, dbflags, paired, P, M))
        _same(res["lean"][0], res["lean"][1], res["full"][0], res["full"][1], ("lean against full", dbflags, paired, P, M))
        sf, sl = res["full"][2], res["lean"][2]
        print("stats", dbflags, paired, P, M, "full", sf, "lean", sl)
        for k in STATS:
            assert sf[k] == sl[k], (k, sf, sl)
        # the hand-over is exercised (and is not the whole batch); the full stage hands nothing on as a lean one
        assert sf["n_lean_queued"] == 0
        assert 0 < sl["n_lean_queued"] < NQ // 2, sl
        # the long lists are among them (12 % of the reads come from the 44-strain species)
        assert sl["n_lean_queued"] > NQ // 50, sl
        # the automatic choice over consecutive batches of a fresh workspace: the first batch runs full, every later one as the
        # counters of the batch before it say.  The calm batch (twice: full, then lean) sets the word, so the mixed batch behind it
        # runs lean and clears it, and the mixed batch behind that runs full again -- results and counts never depend on it
        ws2 = eng.Workspace(db, NQ, max(len(rb), len(calm[paired][0])))
        for i in range(2):
            c, n = ws2.query_host(*calm[paired], paired, max_cand=M, emulate_ranks=P)
            st = ws2.sync()
            _same(c, n, *want_calm[paired, P, M], ("automatic, calm batch %d" % i, dbflags, paired, P, M))
            assert st["n_lean_queued"] * 512 <= NQ, st              # (calm: below the share at which the lean form is entered)
        lean_ran = []
        for i in range(3):
            c, n = ws2.query_host(rb, ro, paired, max_cand=M, emulate_ranks=P)
            st = ws2.sync()
            _same(c, n, oc, on, ("automatic, batch %d" % i, dbflags, paired, P, M))
            for k in STATS:
                assert st[k] == sf[k], ("automatic, batch %d" % i, k, st, sf)
            assert st["n_lean_queued"] in (0, sl["n_lean_queued"]), st
            lean_ran.append(st["n_lean_queued"] != 0)
        assert lean_ran == [AUTO, False, False], lean_ran


def test_forced_flags_are_exclusive_and_checked(world):
    eng, dbbuild, (keys, off, locs, species), single, both, want, calm, want_calm = world
    db = dbbuild.make_database(keys, off, locs, species)
    rb, ro = single
    ws = eng.Workspace(db, NQ, len(rb))
    for qf in (eng.MCQ_FORCE_LEAN_WAVE | eng.MCQ_FORCE_FULL_WAVE,          # both at once
               eng.MCQ_FORCE_LEAN_WAVE | eng.MCQ_FORCE_BLOCK_PATH,         # the lean stage has none of the other test hooks' paths
               eng.MCQ_FORCE_LEAN_WAVE | eng.MCQ_FORCE_RAW_SORT,
               eng.MCQ_FORCE_LEAN_WAVE | eng.MCQ_NO_WAVE16,
               0x80000):                                                   # an unknown bit is still rejected
        with pytest.raises(eng.McqError):
            ws.query_host(rb, ro, False, flags=qf)
    with pytest.raises(eng.McqError):                                      # P x M beyond a wave's lanes: not the lean stage's
        ws.query_host(rb, ro, False, max_cand=4, emulate_ranks=32, flags=eng.MCQ_FORCE_LEAN_WAVE | eng.MCQ_QUIRK_SEQ_DROP | eng.MCQ_FOLD_BY_LISTS)
