"""Which path a query takes, not only what it returns: mcq_stats (Workspace.sync) under the path hooks.

Results are pinned against the oracle elsewhere (test_gpu_scale.py, test_gpu_lean_wave.py); a slip in launch_query's choice of
kernels and hook bits would keep every one of them and only send queries down a slower path.  Here n_overflow -- the queries
that left the first wave stage -- says which way a batch went.  The table of test_gpu_scale.py (6 species x 12 strains, 32-bit
bit fields in 64-B buckets) and 4 000 reads of 150 bases: most are answered by the first wave stage wherever it may."""
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, L = 4000, 150


@pytest.fixture(scope="module")
def world():
    eng = importlib.import_module("metacache-mpi_amd.engine")
    dbbuild = importlib.import_module("dbbuild_torch")
    synth = importlib.import_module("metacache-mpi_amd.synth")
    dev = torch.device("cuda", 0)
    gb, goff, species = synth.make_genomes(6, 12, 200_000, 400_000, 0.02, seed=5, device=dev)
    keys, off, locs, _ = dbbuild.build_table(gb, goff, emulate_ranks=2)
    db = dbbuild.make_database(keys, off, locs, species)
    reads, roff, _ = synth.sample_reads(gb, goff, N, L, 0.01, 0.002, seed=13)
    return eng, db, reads.cpu().numpy().tobytes(), roff.cpu().numpy().astype(np.uint64)


def _run(eng, ws, rb, ro, what, **kw):
    cands, ncand = ws.query_host(rb, ro, False, **kw)
    st = ws.sync()
    print(what, st)
    assert st["n_queries"] == N
    return cands, ncand, st


def test_many_lists_stay_in_the_first_wave_stage(world):
    """P x M beyond a wave's 64 lanes: up to 256 list slots the first wave stage keeps them in registers (`many`) and answers
    queries itself; MCQ_FORCE_BLOCK_PATH, and lists beyond 256 slots, send every query to the workgroup kernel."""
    eng, db, rb, ro = world
    ws = eng.Workspace(db, N, N * L)
    for flags in (0, eng.MCQ_FOLD_BY_LISTS):          # as one selection (the lists fit the lanes again), and as 32 lists of 4
        _, _, st = _run(eng, ws, rb, ro, "P=32 M=4 flags=%x" % flags, max_cand=4, emulate_ranks=32, flags=flags)
        assert st["n_overflow"] < N, st
        _, _, st = _run(eng, ws, rb, ro, "P=32 M=4 block path flags=%x" % flags, max_cand=4, emulate_ranks=32, flags=flags | eng.MCQ_FORCE_BLOCK_PATH)
        assert st["n_overflow"] == N, st
    _, _, st = _run(eng, ws, rb, ro, "P=64 M=16 by lists", max_cand=16, emulate_ranks=64, flags=eng.MCQ_FOLD_BY_LISTS)
    assert st["n_overflow"] == N, st


def test_route_hooks(world):
    """the raw sort changes no route; MCQ_FORCE_BLOCK_PATH sends every query to the workgroup kernel"""
    eng, db, rb, ro = world
    ws = eng.Workspace(db, N, N * L)
    _, _, s0 = _run(eng, ws, rb, ro, "P=2 M=2", max_cand=2, emulate_ranks=2)
    _, _, s1 = _run(eng, ws, rb, ro, "P=2 M=2 raw sort", max_cand=2, emulate_ranks=2, flags=eng.MCQ_FORCE_RAW_SORT)
    _, _, s2 = _run(eng, ws, rb, ro, "P=2 M=2 block path", max_cand=2, emulate_ranks=2, flags=eng.MCQ_FORCE_BLOCK_PATH)
    assert s0["n_overflow"] < N, s0
    assert s1["n_overflow"] == s0["n_overflow"], (s0, s1)
    assert s2["n_overflow"] == N, s2


@pytest.mark.parametrize("hook", ["MCQ_FORCE_BLOCK_PATH", "MCQ_FORCE_RAW_SORT", "MCQ_NO_WAVE16"])
def test_hooks_do_not_persist(world, hook):
    """a batch with a route hook between two plain batches: the last batch goes the way it goes without it (a hook neither
    sets nor survives in the word that tells the next batch how to enter)"""
    eng, db, rb, ro = world
    last = []
    for with_hook in (False, True):
        ws = eng.Workspace(db, N, N * L)
        _run(eng, ws, rb, ro, "first", max_cand=2, emulate_ranks=2)
        if with_hook:
            _run(eng, ws, rb, ro, hook, max_cand=2, emulate_ranks=2, flags=getattr(eng, hook))
        last.append(_run(eng, ws, rb, ro, "last (hook between: %s)" % with_hook, max_cand=2, emulate_ranks=2)[2])
    assert last[0] == last[1], last


def test_lean_form_with_no_two_class(world):
    """MCQ_NO_TWO_CLASS is no route hook: the lean first stage takes it.  Lists beyond a wave's lanes have no lean stage
    (P = 32, M = 4 as 32 lists: MCQ_FOLD_BY_LISTS; as one selection they fit the lanes again and the lean form is accepted)."""
    eng, db, rb, ro = world
    ws = eng.Workspace(db, N, N * L)
    c0, n0, _ = _run(eng, ws, rb, ro, "P=2 M=2", max_cand=2, emulate_ranks=2)
    c1, n1, _ = _run(eng, ws, rb, ro, "P=2 M=2 lean, no two-class", max_cand=2, emulate_ranks=2,
                     flags=eng.MCQ_FORCE_LEAN_WAVE | eng.MCQ_NO_TWO_CLASS)
    assert np.array_equal(n0, n1)
    mask = np.arange(c0.shape[1])[None, :] < n0[:, None]
    assert np.array_equal(c0[mask], c1[mask])
    with pytest.raises(eng.McqError) as e:
        ws.query_host(rb, ro, False, max_cand=4, emulate_ranks=32, flags=eng.MCQ_FORCE_LEAN_WAVE | eng.MCQ_FOLD_BY_LISTS)
    assert e.value.code == eng.MCQ_E_UNSUPPORTED, e.value
