"""The lean first wave stage is compiled for the default sketch geometry (k 16, sketch 16, windows 128 / 113) and for the batch's
form (paired, packed): MCQ_FORCE_LEAN_WAVE against MCQ_FORCE_FULL_WAVE and the CPU oracle on reads whose lengths sit on the k-mer
and window boundaries, in every form a batch can be given in; a table of another geometry has no lean form.

One small table (6 species x 4 strains of 150-300 kb).  The reads' lengths cycle through LENS: below, at and above k = 16, the
window stride 113, the window length 128, 128 + 16, two windows' end 241 (242 is the first read of three windows), and 300 (three
windows, still under 64 features).  Every batch is compared lean against full (n_cand, and cands below n_cand) and against the oracle."""
import importlib
import json
import os

import numpy as np
import pytest
import torch

from oracle import mc_oracle as orc

pytestmark = pytest.mark.gpu

NQ = 4096
LENS = (1, 15, 16, 17, 112, 113, 127, 128, 129, 143, 144, 145, 150, 240, 241, 242, 300)
P, M = 2, 2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lean_geometry_parent_stats.json")
STATS = ("n_features", "n_hit_features", "n_locations", "n_cands", "n_overflow", "n_lean_queued")
GUARD = 0xA5A5A5A5


def boundary_reads(synth, gb, goff, n, seed):
    """n reads sampled from the genomes with the error model of the benchmark's configs[1], read i cut to LENS[i % 17]:
    (bytes, offsets)"""
    src, _, _ = synth.sample_reads(gb, goff, n, 300, 0.005, 0.001, seed=seed)
    src = src.cpu().numpy().reshape(n, 300)
    lens = np.array([LENS[i % len(LENS)] for i in range(n)])
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    return np.concatenate([src[i, :lens[i]] for i in range(n)]).tobytes(), off


def inject_ambiguity(rb, ro, seed):
    """N, IUPAC codes and lower-case bases into every read: anywhere, and inside the last k-mer of the first window and of the read"""
    rng = np.random.default_rng(seed)
    a = np.frombuffer(rb, np.uint8).copy()
    codes = np.frombuffer(b"NRYKMSWBDHVn", np.uint8)
    for i in range(len(ro) - 1):
        o, n = int(ro[i]), int(ro[i + 1] - ro[i])
        kind = i % 4
        if kind == 0:                                   # lower case (still bases)
            m = rng.random(n) < 0.3
            a[o:o + n][m] |= 0x20
        elif kind == 1:                                 # inside the last k-mer of the first window
            a[o + max(0, min(n, 128) - 1 - int(rng.integers(0, 16)))] = codes[int(rng.integers(0, len(codes)))]
        elif kind == 2:                                 # inside the last k-mer of the read (of its last window)
            a[o + max(0, n - 1 - int(rng.integers(0, 16)))] = codes[int(rng.integers(0, len(codes)))]
        else:                                           # a few anywhere, lower case around them
            for _ in range(int(rng.integers(1, 4))):
                p = int(rng.integers(0, n))
                a[o + p] = codes[int(rng.integers(0, len(codes)))]
            a[o:o + n // 2] |= 0x20
    return a.tobytes(), ro


@pytest.fixture(scope="module")
def world():
    """the table, the oracle, the batches and the oracle's answers -- computed once"""
    eng = importlib.import_module("metacache-mpi_amd.engine")
    dbbuild = importlib.import_module("dbbuild_torch")
    synth = importlib.import_module("metacache-mpi_amd.synth")
    dev = torch.device("cuda", 0)
    gb, goff, species = synth.make_genomes(6, 4, 150_000, 300_000, 0.02, seed=31, device=dev)
    keys, off, locs, _ = dbbuild.build_table(gb, goff, emulate_ranks=2)
    db = dbbuild.make_database(keys, off, locs, species)
    host = lambda t, ty: t.cpu().numpy().astype(ty)
    odb = orc.OracleDb(host(keys, np.uint32), host(off, np.uint64), host(locs, np.uint64), host(species, np.uint32))
    single = boundary_reads(synth, gb, goff, NQ, seed=71)
    pairs = boundary_reads(synth, gb, goff, 2 * NQ, seed=72)
    amb = inject_ambiguity(*boundary_reads(synth, gb, goff, NQ, seed=73), seed=74)
    want = {"single": odb.query(*single, False, max_cand=M, emulate_ranks=P, threads=8),
            "pairs": odb.query(*pairs, True, max_cand=M, emulate_ranks=P, threads=8),
            "amb": odb.query(*amb, False, max_cand=M, emulate_ranks=P, threads=8)}
    return dict(eng=eng, dbbuild=dbbuild, synth=synth, dev=dev, gb=gb, goff=goff, species=species, db=db, odb=odb,
                single=single, pairs=pairs, amb=amb, want=want)


def _same(cands, ncand, oc, on, what):
    assert np.array_equal(ncand, on), (what, "n_cand differs at", np.nonzero(ncand != on)[0][:5])
    mask = np.arange(cands.shape[1])[None, :] < on[:, None]
    assert np.array_equal(cands[mask], oc[mask]), (what, "candidate slots differ")


def _lean_full_oracle(w, run, oc, on, what):
    """run(flags) -> (cands, ncand, stats): both forms against the oracle and each other; returns their stats"""
    eng = w["eng"]
    cf, nf, sf = run(eng.MCQ_FORCE_FULL_WAVE)
    cl, nl, sl = run(eng.MCQ_FORCE_LEAN_WAVE)
    _same(cf, nf, oc, on, (what, "full against the oracle"))
    _same(cl, nl, oc, on, (what, "lean against the oracle"))
    _same(cl, nl, cf, nf, (what, "lean against full"))
    for k in ("n_queries", "n_features", "n_hit_features", "n_locations", "n_cands", "n_overflow"):
        assert sf[k] == sl[k], (what, k, sf, sl)
    return sf, sl


def _host_run(w, rb, ro, paired, packed=False):
    ws = w["eng"].Workspace(w["db"], NQ, int(ro[-1]) + 64)           # (rb may be the packed form: fewer bytes than bases)

    def run(flags):
        c, n = ws.query_host(rb, ro, paired, max_cand=M, emulate_ranks=P, flags=flags, packed=packed)
        return c, n, ws.sync()
    return run


def _device_run(w, bases_t, off_t, n_seqs, paired, ranges):
    """device buffers, the outputs followed by guard words that must come back untouched"""
    eng, dev = w["eng"], w["dev"]
    nq = n_seqs // 2 if paired else n_seqs
    ws = eng.Workspace(w["db"], nq, bases_t.numel())
    pad = 4096

    def run(flags):
        cands = torch.full((nq * M * 4 + pad,), GUARD - (1 << 32), dtype=torch.int32, device=dev)
        ncand = torch.full((nq + pad,), GUARD - (1 << 32), dtype=torch.int32, device=dev)
        ws.query_device(bases_t.data_ptr(), off_t.data_ptr(), n_seqs, paired, cands.data_ptr(), ncand.data_ptr(), max_cand=M,
                        emulate_ranks=P, flags=flags, stream=torch.cuda.current_stream(dev).cuda_stream, ranges=ranges)
        st = ws.sync()
        c, n = cands.cpu().numpy().view(np.uint32), ncand.cpu().numpy().view(np.uint32)
        assert (c[nq * M * 4:] == GUARD).all() and (n[nq:] == GUARD).all(), "written behind the outputs"
        return c[:nq * M * 4].reshape(nq, M, 4), n[:nq], st
    return run


def test_single_reads_on_the_boundaries_and_the_parents_counts(world):
    w = world
    rb, ro = w["single"]
    sf, sl = _lean_full_oracle(w, _host_run(w, rb, ro, False), *w["want"]["single"], "single")
    print("stats full", sf, "lean", sl)
    parent = json.load(open(GOLDEN))            # the parent commit's lean form on this batch
    for k in STATS:
        assert sl[k] == parent[k], (k, sl, parent)
    # other list shapes (8 virtual ranks x 4 candidates)
    ws = w["eng"].Workspace(w["db"], NQ, len(rb))
    oc, on = w["odb"].query(rb, ro, False, max_cand=4, emulate_ranks=8, threads=8)
    for qf in (w["eng"].MCQ_FORCE_FULL_WAVE, w["eng"].MCQ_FORCE_LEAN_WAVE):
        c, n = ws.query_host(rb, ro, False, max_cand=4, emulate_ranks=8, flags=qf)
        _same(c, n, oc, on, ("P 8 M 4", qf))


def test_pairs_on_the_boundaries(world):
    w = world
    rb, ro = w["pairs"]
    _lean_full_oracle(w, _host_run(w, rb, ro, True), *w["want"]["pairs"], "pairs")


def test_ambiguous_and_lower_case_bases(world):
    w = world
    rb, ro = w["amb"]
    _lean_full_oracle(w, _host_run(w, rb, ro, False), *w["want"]["amb"], "ambiguous")
    _lean_full_oracle(w, _host_run(w, w["eng"].pack_bases_host(rb), ro, False, packed=True), *w["want"]["amb"], "ambiguous, packed")


def test_packed_batches(world):
    w = world
    eng = w["eng"]
    for name, paired in (("single", False), ("pairs", True)):
        rb, ro = w[name]
        _lean_full_oracle(w, _host_run(w, eng.pack_bases_host(rb), ro, paired, packed=True), *w["want"][name], "packed " + name)


def test_ranges_batch(world):
    """the reads of the single batch as (begin, end) pairs in reverse order"""
    w = world
    rb, ro = w["single"]
    dev = w["dev"]
    bases_t = torch.from_numpy(np.frombuffer(rb, np.uint8).copy()).to(dev)
    order = np.arange(NQ)[::-1]
    rng = np.stack([ro[order], ro[order + 1]], 1).astype(np.int64).reshape(-1)
    off_t = torch.from_numpy(rng).to(dev)
    oc, on = w["want"]["single"]
    _lean_full_oracle(w, _device_run(w, bases_t, off_t, NQ, False, True), oc[order], on[order], "ranges")


@pytest.mark.parametrize("paired", [False, True])
def test_last_read_ends_with_the_buffer(world, paired):
    """device buffers sized exactly: the last read's last base is the buffer's last byte; nothing is written behind the outputs"""
    w = world
    rb, ro = w["pairs" if paired else "single"]
    dev = w["dev"]
    bases_t = torch.empty(len(rb), dtype=torch.uint8, device=dev)
    bases_t.copy_(torch.from_numpy(np.frombuffer(rb, np.uint8).copy()))
    assert bases_t.numel() == int(ro[-1])
    off_t = torch.from_numpy(ro.astype(np.int64)).to(dev)
    _lean_full_oracle(w, _device_run(w, bases_t, off_t, len(ro) - 1, paired, False), *w["want"]["pairs" if paired else "single"], "exact buffer")


@pytest.mark.parametrize("geom", [dict(winlen=100, winstride=85), dict(k=12)])
def test_another_geometry_has_no_lean_form(world, geom):
    w = world
    eng, dbbuild = w["eng"], w["dbbuild"]
    host = lambda t, ty: t.cpu().numpy().astype(ty)
    keys, off, locs, _ = dbbuild.build_table(w["gb"], w["goff"], emulate_ranks=2, **geom)
    db = dbbuild.make_database(keys, off, locs, w["species"], **geom)
    odb = orc.OracleDb(host(keys, np.uint32), host(off, np.uint64), host(locs, np.uint64), host(w["species"], np.uint32), **geom)
    rb, ro = w["single"]
    oc, on = odb.query(rb, ro, False, max_cand=M, emulate_ranks=P, threads=8)
    ws = eng.Workspace(db, NQ, len(rb))
    for i in range(3):              # (on a default table the second batch of a calm workspace runs lean)
        c, n = ws.query_host(rb, ro, False, max_cand=M, emulate_ranks=P)
        st = ws.sync()
        _same(c, n, oc, on, ("automatic, batch %d" % i, geom))
        assert st["n_lean_queued"] == 0, st
    with pytest.raises(eng.McqError) as e:
        ws.query_host(rb, ro, False, max_cand=M, emulate_ranks=P, flags=eng.MCQ_FORCE_LEAN_WAVE)
    assert e.value.code == eng.MCQ_E_UNSUPPORTED and "geometry" in str(e.value), e.value
    c, n = ws.query_host(rb, ro, False, max_cand=M, emulate_ranks=P, flags=eng.MCQ_FORCE_FULL_WAVE)
    _same(c, n, oc, on, ("full", geom))
