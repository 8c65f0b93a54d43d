"""The lean first wave stage's two tails end to end: a read of at most 64 distinct keys, folded as one
selection, with a window range of at most 4 takes narrow_tail_lin (no sort, no sweep); every other read keeps dedup_finish ->
sweep -> top lists.  MCQ_FORCE_LEAN_WAVE against MCQ_FORCE_FULL_WAVE and the CPU oracle: candidates below n_cand, n_cand, and the
six counters of mcq_stats (the comparison itself is test_gpu_lean_loop's).

  insert_size_max   window range   tail of a read with <= 64 distinct keys
  0                 3              sort-free
  300               4              sort-free
  400               5              sorted
  1000              10             sorted (weighted sweep)
P = 1 folds nothing (no single selection): sorted at every range.

Three tables.  SMALL as `bench.py --small` builds it; NINE, test_gpu_lean_loop's one genome entered as nine targets of three taxa;
TIE, one genome entered as four targets of four species -- every hit count occurs four times, on two virtual ranks of two targets each
under P = 2, so the winner of a round is decided by position among different taxa.  What a read hits is the oracle's word: a batch
of NINE or TIE must hold reads of at most 64 distinct keys, reads of more (among those of at most 256 locations, which the stage
keeps) and reads without a location before it is used.  SMALL's genomes are random: a read there meets its species' four strains in
two or three windows, a dozen keys -- its batches are asked for the first and the last kind only."""
import importlib

import numpy as np
import pytest
import torch

from oracle import mc_oracle as orc
from test_gpu_lean_loop import KEEP_LEAN, READ, STRIDE, Table, _check, _host_run, nine_genome, nine_reads, nine_table

pytestmark = pytest.mark.gpu

NQ = 1200                                      # queries per batch: at most 2400 reads of 150 bp


def tie_genome(seed):
    """random | 339 bases x 12 | random, 113 n + 37 bases in all: a read inside the repeat meets 12 windows per window of its own --
    with four targets more than 64 distinct keys, at 48 locations per feature; (bytes, start of the repeat)"""
    rng = np.random.default_rng(seed)
    rnd = lambda n: rng.integers(0, 4, n)
    parts = [rnd(4007), np.tile(rnd(3 * STRIDE), 12), rnd(1500)]
    g = np.concatenate(parts)
    g = np.concatenate([g, rnd((37 - len(g)) % STRIDE)])
    return np.frombuffer(b"ACGT", np.uint8)[g].tobytes(), len(parts[0])


def batch_kinds(odb, reads, nq, paired):
    """(locations, distinct keys) of the batch's first nq queries, by the oracle"""
    m = [odb.matches(r) for r in reads[:2 * nq if paired else nq]]
    if paired:
        m = [np.concatenate([m[2 * i], m[2 * i + 1]]) for i in range(nq)]
    return np.array([len(x) for x in m]), np.array([len(np.unique(x)) for x in m])


def assert_kinds(T, D, wide, what):
    kept = (T > 0) & (T <= KEEP_LEAN)
    assert (kept & (D <= 64)).any(), (what, "no kept read with at most 64 distinct keys")
    assert (T == 0).any(), (what, "no read without a location")
    if wide:
        assert (kept & (D > 64)).any(), (what, "no kept read with more than 64 distinct keys", sorted(set(D[kept].tolist()))[-5:])


@pytest.fixture(scope="module")
def world():
    eng = importlib.import_module("metacache-mpi_amd.engine")
    dbbuild = importlib.import_module("dbbuild_torch")
    synth = importlib.import_module("metacache-mpi_amd.synth")
    dev = torch.device("cuda", 0)
    n_seqs = 2 * NQ
    host = lambda t, ty: t.cpu().numpy().astype(ty)
    gb, goff, species = synth.make_genomes(6, 4, 150_000, 300_000, 0.02, seed=31, device=dev)
    keys, off, locs, _ = dbbuild.build_table(gb, goff, emulate_ranks=2)
    db = dbbuild.make_database(keys, off, locs, species)
    odb = orc.OracleDb(host(keys, np.uint32), host(off, np.uint64), host(locs, np.uint64), host(species, np.uint32))
    rd, _, _ = synth.sample_reads(gb, goff, n_seqs, READ, 0.005, 0.001, seed=191)
    rd = rd.cpu().numpy().reshape(n_seqs, READ)
    rng = np.random.default_rng(192)
    rnd_pair = (np.arange(n_seqs) // 2) % 7 == 0              # both mates of every seventh pair: random bases
    rd[rnd_pair] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (int(rnd_pair.sum()), READ))]
    tabs = {"small": (Table(db, odb, [r.tobytes() for r in rd]), False)}
    genome, at4, at8 = nine_genome(93)
    k9, o9, l9, t9 = nine_table(genome)
    pool = nine_reads(genome, at4, at8, 94)
    tabs["nine"] = (Table(eng.Database(k9, o9, l9, t9), orc.OracleDb(k9, o9, l9, t9), [pool[i % len(pool)] for i in range(n_seqs)]), True)
    tg, at = tie_genome(95)
    k4, o4, l4, _ = nine_table(tg, copies=4)
    t4 = np.array([11, 12, 13, 14], np.uint32)                  # four species
    # pair j is two neighbours of the pool, (7 j, 7 j + 1): the pool ends with four random reads, so some pairs hit nothing
    pool4 = nine_reads(tg, at, at, 96)
    tabs["tie"] = (Table(eng.Database(k4, o4, l4, t4), orc.OracleDb(k4, o4, l4, t4),
                         [pool4[(7 * (i // 2) + (i & 1)) % len(pool4)] for i in range(n_seqs)]), True)
    kinds = {}
    for name, (tab, wide) in tabs.items():
        reads = [tab.bases[int(tab.off[i]):int(tab.off[i + 1])] for i in range(tab.n)]
        for paired in (False, True):
            T, D = batch_kinds(tab.odb, reads, NQ, paired)
            assert_kinds(T, D, wide, (name, "paired" if paired else "single"))
            kinds[name, paired] = (T, D)
    yield dict(eng=eng, dev=dev, tabs={k: v[0] for k, v in tabs.items()}, kinds=kinds, keep=(gb, keys, off, locs, species))


@pytest.mark.parametrize("paired,packed", [(False, False), (True, False), (False, True)])
@pytest.mark.parametrize("ism", [0, 300, 400, 1000])
@pytest.mark.parametrize("table", ["small", "nine", "tie"])
def test_window_ranges(world, table, ism, paired, packed):
    """ranges of 3 and 4 windows: the sort-free tail; 5 and 10: the sorted one -- single reads, pairs, packed bases"""
    w = world
    tab = w["tabs"][table]
    _check(w, tab, NQ, paired, _host_run(w, tab, NQ, paired, 2, 2, ism, packed=packed),
           "%s, insert_size_max %d, paired %d packed %d" % (table, ism, paired, packed), M=2, P=2, ism=ism)


@pytest.mark.parametrize("P", [1, 2, 3, 4])
@pytest.mark.parametrize("M", [1, 2, 4])
@pytest.mark.parametrize("table", ["small", "nine", "tie"])
def test_list_shapes(world, table, M, P):
    """no fold (the sorted tail), one selection over two and four ranks, three ranks of which the third is dropped -- at both narrow ranges"""
    w = world
    tab = w["tabs"][table]
    for ism in (0, 300):
        _check(w, tab, NQ, False, _host_run(w, tab, NQ, False, M, P, ism), "%s, M %d P %d, insert_size_max %d" % (table, M, P, ism), M=M, P=P, ism=ism)
