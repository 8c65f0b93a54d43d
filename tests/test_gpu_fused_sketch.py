"""The lean first wave stage sketches a single read of 129..160 bases in one pass over both its windows (wave_sketch_two_windows);
every other length keeps the loop over the windows.  MCQ_FORCE_LEAN_WAVE against MCQ_FORCE_FULL_WAVE (which sketches window by
window) and the CPU oracle, end to end, on the small table of test_gpu_lean_geometry.py (6 species x 4 strains).

The reads' lengths cycle through LENS: 128 and 161 on either side of the one-pass range, its ends 129 and 160, 143 / 144 / 145
around a second window of 16 k-mers, 150 and 151 as sequencers write them.  A second batch mixes in ambiguity codes and lower case
on the boundaries of the two windows, windows with few k-mers and tandem repeats.  Batches are given as host buffers, as device
buffers (sized exactly) and as ranges."""
import importlib

import numpy as np
import pytest
import torch

from oracle import mc_oracle as orc

pytestmark = pytest.mark.gpu

NQ = 4096
LENS = (128, 129, 130, 143, 144, 145, 150, 151, 159, 160, 161)
P, M = 2, 2
STATS = ("n_queries", "n_features", "n_hit_features", "n_locations", "n_cands", "n_overflow")
GUARD = 0xA5A5A5A5


def cut_reads(synth, gb, goff, n, seed):
    """n reads sampled from the genomes with the error model of the benchmark's configs[1], read i cut to LENS[i % 11]"""
    src, _, _ = synth.sample_reads(gb, goff, n, 161, 0.005, 0.001, seed=seed)
    src = src.cpu().numpy().reshape(n, 161)
    lens = np.array([LENS[i % len(LENS)] for i in range(n)])
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    return np.concatenate([src[i, :lens[i]] for i in range(n)]).tobytes(), off


def inject_patterns(rb, ro, seed):
    """per read one of: lower case; a code in the last k-mer of the first window (bases 112..127), in the k-mer at 113, in the
    read's last k-mer; Ns that leave the first window at most 32 or 33..64 k-mers; a tandem repeat of period 4; all N;
    nothing (13 kinds against 11 lengths: every kind meets every length)"""
    rng = np.random.default_rng(seed)
    a = np.frombuffer(rb, np.uint8).copy()
    codes = np.frombuffer(b"NRYKMSWBDHVn", np.uint8)
    code = lambda: codes[int(rng.integers(0, len(codes)))]
    for i in range(len(ro) - 1):
        o, n = int(ro[i]), int(ro[i + 1] - ro[i])
        r = a[o:o + n]
        kind = i % 13
        if kind == 0:
            r[rng.random(n) < 0.3] |= 0x20
        elif kind == 1:
            r[112 + int(rng.integers(0, 16))] = code()
        elif kind == 2:
            r[min(n - 1, 113 + int(rng.integers(0, 16)))] = code()
        elif kind == 3:
            r[n - 1 - int(rng.integers(0, 16))] = code()
        elif kind == 4:                                 # one clean stretch of 16..47 bases in the first window: 1..32 k-mers
            ln = 16 + int(rng.integers(0, 32)); at = int(rng.integers(0, 128 - ln + 1))
            r[:at] = ord("N"); r[at + ln:128] = ord("N")
        elif kind == 5:                                 # ... of 48..79 bases: 33..64 k-mers
            ln = 48 + int(rng.integers(0, 32)); at = int(rng.integers(0, 128 - ln + 1))
            r[:at] = ord("N"); r[at + ln:128] = ord("N")
        elif kind == 6:                                 # the first window is a tandem repeat of period 4 (113 k-mers, few hashes)
            r[:113] = np.resize(r[:4], 113)
        elif kind == 7:
            r[:] = np.resize(r[:4], n)
        elif kind == 8:
            r[:] = ord("N")
        elif kind == 9:                                 # lower case around a few codes anywhere
            for _ in range(int(rng.integers(1, 4))):
                r[int(rng.integers(0, n))] = code()
            r[:n // 2] |= 0x20
    return a.tobytes(), ro


@pytest.fixture(scope="module")
def world():
    """the table, the oracle, the two batches and the oracle's answers -- computed once"""
    eng = importlib.import_module("metacache-mpi_amd.engine")
    dbbuild = importlib.import_module("dbbuild_torch")
    synth = importlib.import_module("metacache-mpi_amd.synth")
    dev = torch.device("cuda", 0)
    gb, goff, species = synth.make_genomes(6, 4, 150_000, 300_000, 0.02, seed=31, device=dev)
    keys, off, locs, _ = dbbuild.build_table(gb, goff, emulate_ranks=2)
    db = dbbuild.make_database(keys, off, locs, species)
    host = lambda t, ty: t.cpu().numpy().astype(ty)
    odb = orc.OracleDb(host(keys, np.uint32), host(off, np.uint64), host(locs, np.uint64), host(species, np.uint32))
    plain = cut_reads(synth, gb, goff, NQ, seed=81)
    mixed = inject_patterns(*cut_reads(synth, gb, goff, NQ, seed=82), seed=83)
    want = {"plain": odb.query(*plain, False, max_cand=M, emulate_ranks=P, threads=8),
            "mixed": odb.query(*mixed, False, max_cand=M, emulate_ranks=P, threads=8)}
    return dict(eng=eng, dev=dev, db=db, plain=plain, mixed=mixed, want=want)


def _same(cands, ncand, oc, on, what):
    assert np.array_equal(ncand, on), (what, "n_cand differs at", np.nonzero(ncand != on)[0][:5])
    mask = np.arange(cands.shape[1])[None, :] < on[:, None]
    assert np.array_equal(cands[mask], oc[mask]), (what, "candidate slots differ")


def _lean_full_oracle(w, run, oc, on, what):
    """run(flags) -> (cands, ncand, stats): both forms against the oracle and each other, and their counters"""
    eng = w["eng"]
    cf, nf, sf = run(eng.MCQ_FORCE_FULL_WAVE)
    cl, nl, sl = run(eng.MCQ_FORCE_LEAN_WAVE)
    print(what, "full", {k: sf[k] for k in STATS}, "lean", {k: sl[k] for k in STATS})
    _same(cf, nf, oc, on, (what, "full against the oracle"))
    _same(cl, nl, oc, on, (what, "lean against the oracle"))
    _same(cl, nl, cf, nf, (what, "lean against full"))
    for k in STATS:
        assert sf[k] == sl[k], (what, k, sf, sl)


def _host_run(w, rb, ro):
    ws = w["eng"].Workspace(w["db"], NQ, int(ro[-1]) + 64)

    def run(flags):
        c, n = ws.query_host(rb, ro, False, max_cand=M, emulate_ranks=P, flags=flags)
        return c, n, ws.sync()
    return run


def _device_run(w, bases_t, off_t, ranges):
    """device buffers, the outputs followed by guard words that must come back untouched"""
    eng, dev = w["eng"], w["dev"]
    ws = eng.Workspace(w["db"], NQ, bases_t.numel())
    pad = 4096

    def run(flags):
        cands = torch.full((NQ * M * 4 + pad,), GUARD - (1 << 32), dtype=torch.int32, device=dev)
        ncand = torch.full((NQ + pad,), GUARD - (1 << 32), dtype=torch.int32, device=dev)
        ws.query_device(bases_t.data_ptr(), off_t.data_ptr(), NQ, False, cands.data_ptr(), ncand.data_ptr(), max_cand=M,
                        emulate_ranks=P, flags=flags, stream=torch.cuda.current_stream(dev).cuda_stream, ranges=ranges)
        st = ws.sync()
        c, n = cands.cpu().numpy().view(np.uint32), ncand.cpu().numpy().view(np.uint32)
        assert (c[NQ * M * 4:] == GUARD).all() and (n[NQ:] == GUARD).all(), "written behind the outputs"
        return c[:NQ * M * 4].reshape(NQ, M, 4), n[:NQ], st
    return run


@pytest.mark.parametrize("batch", ["plain", "mixed"])
def test_host_buffers(world, batch):
    w = world
    rb, ro = w[batch]
    _lean_full_oracle(w, _host_run(w, rb, ro), *w["want"][batch], batch + ", host buffers")


@pytest.mark.parametrize("batch", ["plain", "mixed"])
def test_device_buffers_sized_exactly(world, batch):
    """the last read's last base is the buffer's last byte"""
    w = world
    rb, ro = w[batch]
    bases_t = torch.empty(len(rb), dtype=torch.uint8, device=w["dev"])
    bases_t.copy_(torch.from_numpy(np.frombuffer(rb, np.uint8).copy()))
    assert bases_t.numel() == int(ro[-1])
    off_t = torch.from_numpy(ro.astype(np.int64)).to(w["dev"])
    _lean_full_oracle(w, _device_run(w, bases_t, off_t, False), *w["want"][batch], batch + ", device buffers")


@pytest.mark.parametrize("batch", ["plain", "mixed"])
def test_ranges(world, batch):
    """the reads as (begin, end) pairs in reverse order"""
    w = world
    rb, ro = w[batch]
    bases_t = torch.from_numpy(np.frombuffer(rb, np.uint8).copy()).to(w["dev"])
    order = np.arange(NQ)[::-1]
    rng = np.stack([ro[order], ro[order + 1]], 1).astype(np.int64).reshape(-1)
    off_t = torch.from_numpy(rng).to(w["dev"])
    oc, on = w["want"][batch]
    _lean_full_oracle(w, _device_run(w, bases_t, off_t, True), oc[order], on[order], batch + ", ranges")
