"""The lean first wave stage's per-read loop: a 32-bit read index and stride, 32-bit statistics folded into the 64-bit counters when
the kernel ends, the window-range width from a launch constant, the two sequence offsets by scalar loads.
MCQ_FORCE_LEAN_WAVE against MCQ_FORCE_FULL_WAVE and the CPU oracle: candidates below n_cand, n_cand, and every counter of mcq_stats.

Two tables.  SMALL is the one `bench.py --small` builds (6 species x 4 strains of 150-300 kb).  NINE is one genome of 13 kb entered
as 9 targets: a feature's list holds 9 locations, 36 inside the genome's stretch of period 339 = 3 strides repeated 4 times, 72
inside the one repeated 8 times.  The genome is 113 n + 37 bases long, so its last 150 bases are a full window and the short last
window: all 32 features of that read hit, 288 locations.  Reads are cut from there and from the repeats with their first x and last
y bases replaced by random ones, which takes features away; what a read hits is the oracle's word (OracleDb.matches), and the test
asks that the batch holds one read of every kind before it uses it:
  locations   0 | 1-64 | 65-128 | 129-192 | 193-256 (one gather width each) | 257-512 (handed on; the full form keeps them) | > 512
  distinct    <= 32 | 33-64 | > 64 keys among the reads of at most 256 locations (one sort width each; > 64: the weighted sweep)

The first stage's grid is the resident workgroups, which a workspace does not report; MCQ_WAVE_BLOCKS_PER_CU = 1 fixes it at one
workgroup of four waves per compute unit, so W = 4 x compute units, and the batch sizes around the index arithmetic are 1, 3, 5,
W - 1, W + 1 and 3 W + 5."""
import importlib
import os

import numpy as np
import pytest
import torch

from oracle import mc_oracle as orc

pytestmark = pytest.mark.gpu

STATS = ("n_features", "n_hit_features", "n_locations", "n_cands", "n_overflow", "n_lean_queued")
GUARD = 0xA5A5A5A5
STRIDE, WINLEN, READ = 113, 128, 150
KEEP_LEAN, KEEP_FULL = 256, 512            # the longest list the lean / the full first stage answers itself


def nine_genome(seed):
    """13 kb: random | 339 bases x 4 | random | 339 bases x 8 | random, 113 n + 37 bases in all; (bytes, start of x4, start of x8)"""
    rng = np.random.default_rng(seed)
    rnd = lambda n: rng.integers(0, 4, n)
    parts = [rnd(5989), np.tile(rnd(3 * STRIDE), 4), rnd(1469), np.tile(rnd(3 * STRIDE), 8), rnd(1500)]
    g = np.concatenate(parts)
    g = np.concatenate([g, rnd((37 - len(g)) % STRIDE)])
    assert len(g) % STRIDE == 37
    return np.frombuffer(b"ACGT", np.uint8)[g].tobytes(), len(parts[0]), len(parts[0]) + len(parts[1]) + len(parts[2])


def nine_table(genome, copies=9):
    """the union table of `copies` identical targets, built on the CPU with the oracle's sketch: (keys, list_off, locs, tgt2tax)"""
    per_feature = {}
    for j, (b, e) in enumerate(orc.windows(len(genome), WINLEN, STRIDE)):
        for f in orc.sketch(genome[b:e]):
            per_feature.setdefault(int(f), []).append(j)
    keys = np.array(sorted(per_feature), np.uint32)
    lists = [np.array([(t << 32) | j for t in range(copies) for j in per_feature[int(f)]], np.uint64) for f in keys]
    off = np.zeros(len(keys) + 1, np.uint64)
    off[1:] = np.cumsum([len(l) for l in lists])
    return keys, off, np.concatenate(lists), np.array([1 + t // 3 for t in range(copies)], np.uint32)     # three taxa of three targets


def nine_reads(genome, at4, at8, seed):
    """the candidate reads: the genome's last 150 bases, and reads on the windows of the two repeats, each with its first x and
    last y bases replaced by random ones; random reads"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    g = np.frombuffer(genome, np.uint8)
    first = lambda at: -(-at // STRIDE) * STRIDE              # the first window that starts inside a repeat
    out = []
    for start, xs, ys in ((len(g) - READ, range(0, 120, 6), (0, 8, 16, 24, 37)),
                          (first(at4) + 3 * STRIDE, range(0, 120, 6), (0, 37)),
                          (first(at8) + 6 * STRIDE, range(0, 120, 6), (0, 37)),
                          (1000 + 57, (0, 30), (0,))):
        for x in xs:
            for y in ys:
                r = g[start:start + READ].copy()
                r[:x] = acgt[rng.integers(0, 4, x)]
                r[READ - y:] = acgt[rng.integers(0, 4, y)]
                out.append(r.tobytes())
    out += [acgt[rng.integers(0, 4, READ)].tobytes() for _ in range(4)]
    return out


def kinds_of(odb, reads):
    """(locations, distinct keys) of every read, by the oracle"""
    m = [odb.matches(r) for r in reads]
    return np.array([len(x) for x in m]), np.array([len(np.unique(x)) for x in m])


def assert_every_kind(T, D):
    for lo, hi in ((0, 0), (1, 64), (65, 128), (129, 192), (193, 256), (257, 512), (513, 1 << 30)):
        assert ((T >= lo) & (T <= hi)).any(), ("no read with %d..%d locations" % (lo, hi), sorted(set(T.tolist())))
    kept = T <= KEEP_LEAN
    for lo, hi in ((1, 32), (33, 64), (65, 256)):
        assert (kept & (D >= lo) & (D <= hi)).any(), ("no kept read with %d..%d distinct keys" % (lo, hi), sorted(set(D[kept].tolist())))
    assert (T == 288).any(), "the read of 32 features x 9 locations is missing"


class Table:
    """a table on the device, its oracle, a batch of single reads and one of pairs (the same bytes read two by two), and how many
    locations each query has"""

    def __init__(self, db, odb, reads):
        self.db, self.odb = db, odb
        self.bases, self.off = orc.pack_reads(reads)
        self.n = len(reads)
        T1, _ = kinds_of(odb, reads)
        self.T = {False: T1, True: T1[0::2][:self.n // 2] + T1[1::2][:self.n // 2]}

    def batch(self, nq, paired):
        n_seqs = 2 * nq if paired else nq
        assert n_seqs <= self.n
        return self.bases[:int(self.off[n_seqs])], self.off[:n_seqs + 1]


@pytest.fixture(scope="module")
def world():
    eng = importlib.import_module("metacache-mpi_amd.engine")
    dbbuild = importlib.import_module("dbbuild_torch")
    synth = importlib.import_module("metacache-mpi_amd.synth")
    dev = torch.device("cuda", 0)
    W = 4 * torch.cuda.get_device_properties(dev).multi_processor_count
    nmax = 3 * W + 5
    n_seqs = nmax + (nmax & 1)                  # (enough for W + 1 pairs too)
    host = lambda t, ty: t.cpu().numpy().astype(ty)
    # SMALL: reads drawn like the benchmark's, every seventh one random bases
    gb, goff, species = synth.make_genomes(6, 4, 150_000, 300_000, 0.02, seed=31, device=dev)
    keys, off, locs, _ = dbbuild.build_table(gb, goff, emulate_ranks=2)
    db = dbbuild.make_database(keys, off, locs, species)
    odb = orc.OracleDb(host(keys, np.uint32), host(off, np.uint64), host(locs, np.uint64), host(species, np.uint32))
    rd, _, _ = synth.sample_reads(gb, goff, n_seqs, READ, 0.005, 0.001, seed=91)
    rd = rd.cpu().numpy().reshape(n_seqs, READ)
    rng = np.random.default_rng(92)
    rd[::7] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (len(rd[::7]), READ))]
    small = Table(db, odb, [r.tobytes() for r in rd])
    assert (small.T[False] == 0).any() and (small.T[False] > 0).any()
    # NINE: every kind of read, in turn
    genome, at4, at8 = nine_genome(93)
    k9, o9, l9, t9 = nine_table(genome)
    pool = nine_reads(genome, at4, at8, 94)
    odb9 = orc.OracleDb(k9, o9, l9, t9)
    assert_every_kind(*kinds_of(odb9, pool))
    nine = Table(eng.Database(k9, o9, l9, t9), odb9, [pool[i % len(pool)] for i in range(n_seqs)])
    old = os.environ.get("MCQ_WAVE_BLOCKS_PER_CU")
    os.environ["MCQ_WAVE_BLOCKS_PER_CU"] = "1"           # read when a workspace is created
    try:
        yield dict(eng=eng, dev=dev, W=W, small=small, nine=nine, keep=(gb, keys, off, locs, species))
    finally:
        if old is None:
            del os.environ["MCQ_WAVE_BLOCKS_PER_CU"]
        else:
            os.environ["MCQ_WAVE_BLOCKS_PER_CU"] = old


def _same(cands, ncand, oc, on, what):
    assert np.array_equal(ncand, on), (what, "n_cand differs at", np.nonzero(ncand != on)[0][:5])
    mask = np.arange(cands.shape[1])[None, :] < on[:, None]
    assert np.array_equal(cands[mask], oc[mask]), (what, "candidate slots differ")


def _check(w, tab, nq, paired, run, what, M=2, P=2, ism=0):
    """run(flags) -> (cands, ncand, stats).  Both forms against the oracle and each other; the counters against the oracle's and
    against what the oracle's match counts say about the queues"""
    eng = w["eng"]
    rb, ro = tab.batch(nq, paired)
    oc, on, ost = tab.odb.query(rb, ro, paired, max_cand=M, emulate_ranks=P, insert_size_max=ism, threads=8, want_stats=True)
    T = tab.T[paired][:nq]
    want = dict(n_features=int(ost[0]), n_hit_features=int(ost[1]), n_locations=int(ost[2]), n_cands=int(ost[3]),
                n_overflow=int((T > KEEP_FULL).sum()))
    cf, nf, sf = run(eng.MCQ_FORCE_FULL_WAVE)
    cl, nl, sl = run(eng.MCQ_FORCE_LEAN_WAVE)
    print(what, "oracle", want, "full", {k: sf[k] for k in STATS}, "lean", {k: sl[k] for k in STATS})
    _same(cf, nf, oc, on, (what, "full against the oracle"))
    _same(cl, nl, oc, on, (what, "lean against the oracle"))
    _same(cl, nl, cf, nf, (what, "lean against full"))
    assert sf["n_queries"] == nq and sl["n_queries"] == nq, (what, sf, sl)
    for k, v in want.items():
        assert sl[k] == v, (what, "lean", k, sl, want)
        assert sf[k] == v, (what, "full", k, sf, want)
    assert sf["n_lean_queued"] == 0, (what, sf)
    assert sl["n_lean_queued"] == int(((T > KEEP_LEAN) & (T <= KEEP_FULL)).sum()), (what, sl)


def _host_run(w, tab, nq, paired, M, P, ism, packed=False):
    eng = w["eng"]
    rb, ro = tab.batch(nq, paired)
    ws = eng.Workspace(tab.db, nq, int(ro[-1]) + 64)
    bases = eng.pack_bases_host(rb) if packed else rb

    def run(flags):
        c, n = ws.query_host(bases, ro, paired, max_cand=M, emulate_ranks=P, insert_size_max=ism, flags=flags, packed=packed)
        return c, n, ws.sync()
    return run


def _device_run(w, tab, nq, paired, M, P, ism):
    """device buffers; the outputs are exactly nq x M x 4 and nq words, and the guard words behind them come back untouched"""
    eng, dev = w["eng"], w["dev"]
    rb, ro = tab.batch(nq, paired)
    bases_t = torch.from_numpy(np.frombuffer(rb, np.uint8).copy()).to(dev)
    off_t = torch.from_numpy(ro.astype(np.int64)).to(dev)
    ws = eng.Workspace(tab.db, nq, bases_t.numel())
    pad = 1024

    def run(flags):
        cands = torch.full((nq * M * 4 + pad,), GUARD - (1 << 32), dtype=torch.int32, device=dev)
        ncand = torch.full((nq + pad,), GUARD - (1 << 32), dtype=torch.int32, device=dev)
        ws.query_device(bases_t.data_ptr(), off_t.data_ptr(), len(ro) - 1, paired, cands.data_ptr(), ncand.data_ptr(), max_cand=M,
                        emulate_ranks=P, insert_size_max=ism, flags=flags, stream=torch.cuda.current_stream(dev).cuda_stream)
        st = ws.sync()
        c, n = cands.cpu().numpy().view(np.uint32), ncand.cpu().numpy().view(np.uint32)
        assert (c[nq * M * 4:] == GUARD).all() and (n[nq:] == GUARD).all(), "written behind the outputs"
        return c[:nq * M * 4].reshape(nq, M, 4), n[:nq], st
    return run


@pytest.mark.parametrize("table", ["small", "nine"])
def test_batch_sizes_around_the_stride(world, table):
    """one read, fewer reads than a workgroup has waves, one more; one wave idle, one wave with a second read; three rounds and five"""
    w = world
    tab, W = w[table], w["W"]
    for nq in (1, 3, 5, W - 1, W + 1, 3 * W + 5):
        _check(w, tab, nq, False, _device_run(w, tab, nq, False, 2, 2, 0), "%s, %d reads" % (table, nq))


@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("ism", [0, 150, 1000, 1 << 33])
@pytest.mark.parametrize("table", ["small", "nine"])
def test_insert_size_max(world, table, ism, paired):
    """0 and 150: the read's length decides; 1000: a window range wider than 8, the weighted sweep; 2^33: range_width's 64-bit branch"""
    w = world
    tab, nq = w[table], w["W"] + 1
    _check(w, tab, nq, paired, _host_run(w, tab, nq, paired, 2, 2, ism), "%s, insert_size_max %d, paired %d" % (table, ism, paired), ism=ism)


@pytest.mark.parametrize("P", [1, 2, 3])
@pytest.mark.parametrize("M", [1, 2, 4])
@pytest.mark.parametrize("table", ["small", "nine"])
def test_list_shapes(world, table, M, P):
    """one selection, lists with a fold, a number of virtual ranks that is no power of two"""
    w = world
    tab, nq = w[table], w["W"] + 1
    _check(w, tab, nq, False, _host_run(w, tab, nq, False, M, P, 0), "%s, M %d P %d" % (table, M, P), M=M, P=P)


@pytest.mark.parametrize("paired,packed", [(False, True), (True, False), (True, True)])
@pytest.mark.parametrize("table", ["small", "nine"])
def test_packed_and_paired_forms(world, table, paired, packed):
    w = world
    tab, nq = w[table], w["W"] + 1
    _check(w, tab, nq, paired, _host_run(w, tab, nq, paired, 2, 2, 0, packed=packed), "%s, paired %d packed %d" % (table, paired, packed))
    if paired and not packed:       # pairs through device buffers sized exactly as well
        _check(w, tab, nq, True, _device_run(w, tab, nq, True, 2, 2, 0), "%s, pairs, device buffers" % table)
