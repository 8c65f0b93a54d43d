"""mcq_range_build_*: the union table of mcq_build_table, one feature-hash range at a time.  The tables of all ranges together
must be the one-piece table: the same keys, every key with the identical list; a range holds exactly the keys whose hash falls
into it, in ascending order.  Everything is an equality."""
import importlib

import numpy as np
import pytest

from ambig_ref import numpy_filter
from test_gpu_build_cli import _numpy_split

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    import torch
    pkg = importlib.import_module("metacache-mpi_amd")
    return pkg, importlib.import_module("metacache-mpi_amd.engine"), importlib.import_module("metacache-mpi_amd.synth"), torch


@pytest.fixture(scope="module")
def genomes(mods):
    pkg, eng, synth, torch = mods
    gb, goff, species = synth.make_genomes(300, 10, 2000, 3000, 0.02, seed=11, device=torch.device("cuda", 0))
    assert goff.numel() - 1 == 3000
    return gb, goff, species.cpu().numpy().astype(np.uint32)


_one_piece = {}


def _reference(eng, genomes, P, flags, max_locs):
    """mcq_build_table's arrays on the host, built once per parameter set and left unchanged"""
    key = (P, flags, max_locs)
    if key not in _one_piece:
        gb, goff, _ = genomes
        t = eng.Table(gb.data_ptr(), goff.data_ptr(), goff.numel() - 1, emulate_ranks=P, max_locs=max_locs, device=0, flags=flags)
        _one_piece[key] = t.to_host() + (t.tgt_windows(),)
        for a in _one_piece[key]:
            a.setflags(write=False)
        t.close()
    return _one_piece[key]


def _tmh(x):
    """thomas_mueller_hash on uint32 arrays (what mcq_owner and the feature ranges use)"""
    x = x.astype(np.uint64)
    for _ in range(2):
        x = (((x >> np.uint64(16)) ^ x) * np.uint64(0x45d9f3b)) & np.uint64(0xFFFFFFFF)
    return (x >> np.uint64(16)) ^ x


def _range_tables(eng, genomes, n_ranges, P, flags, max_locs, win_off):
    """the host arrays of every range's table (checked: the range's keys only, ascending; win_off over all targets), and tgt_windows"""
    gb, goff, _ = genomes
    rb = eng.RangeBuild(gb.data_ptr(), goff.data_ptr(), goff.numel() - 1, n_ranges=n_ranges, emulate_ranks=P, max_locs=max_locs,
                        device=0, flags=flags)
    assert rb.n_ranges == n_ranges and rb.n_windows == int(win_off[-1])
    windows = rb.tgt_windows()
    out = []
    for r, t in enumerate(rb):
        keys, off, locs, w = t.to_host()
        assert t.n_targets == goff.numel() - 1 and np.array_equal(w, win_off)
        assert np.array_equal((_tmh(keys) * np.uint64(n_ranges)) >> np.uint64(32), np.full(len(keys), r, np.uint64)), r
        assert (np.diff(keys.astype(np.int64)) > 0).all() and off[0] == 0 and int(off[-1]) == len(locs) and (np.diff(off.astype(np.int64)) > 0).all()
        out.append((keys, off, locs))
        t.close()
    assert len(out) == n_ranges
    with pytest.raises(StopIteration):
        next(rb)
    rb.close()
    return out, windows


def _sorted_union(tables):
    """the tables' keys together in ascending order, every key with its list"""
    keys = np.concatenate([k for k, _, _ in tables])
    lens = np.concatenate([np.diff(o.astype(np.int64)) for _, o, _ in tables])
    locs = np.concatenate([l for _, _, l in tables])
    order = np.argsort(keys, kind="stable")
    starts = np.cumsum(lens) - lens
    lo = lens[order]
    idx = np.repeat(starts[order], lo) + (np.arange(int(lo.sum()), dtype=np.int64) - np.repeat(np.cumsum(lo) - lo, lo))
    off = np.zeros(len(keys) + 1, np.uint64)
    off[1:] = np.cumsum(lo)
    return keys[order], off, locs[idx]


def _check_equal(eng, genomes, n_ranges, P, flags, max_locs):
    keys, off, locs, win_off, windows = _reference(eng, genomes, P, flags, max_locs)
    tables, w = _range_tables(eng, genomes, n_ranges, P, flags, max_locs, win_off)
    assert np.array_equal(w, windows)
    k2, o2, l2 = tables[0] if n_ranges == 1 else _sorted_union(tables)       # (one range: equal without sorting)
    assert np.array_equal(k2, keys) and np.array_equal(o2, off) and np.array_equal(l2, locs), (n_ranges, P, flags, max_locs)
    return tables


@pytest.mark.parametrize("flags,max_locs", [(0, 0), ("overpop", 0), ("overpop", 3), (0, 3)])
@pytest.mark.parametrize("P", [1, 3, 8])
def test_the_ranges_together_are_the_one_piece_table(mods, genomes, P, flags, max_locs):
    """max_locs = 3 beside the default 254: ten strains per species never reach 254, so only there the per-(feature, rank) limit and
    -remove-overpopulated-features take anything away"""
    pkg, eng, synth, torch = mods
    flags = eng.MCQ_BUILD_REMOVE_OVERPOPULATED if flags else 0
    ref = _reference(eng, genomes, P, flags, max_locs)
    assert len(ref[0]) > 100000
    if max_locs and (flags or P < 8):       # (the ten strains of a species are consecutive targets: at P = 8 no rank holds more than two)
        plain = _reference(eng, genomes, P, 0, 0)
        assert len(ref[2]) < len(plain[2]) and (not flags or len(ref[0]) < len(plain[0]))
    for n_ranges in (1, 2, 5):
        _check_equal(eng, genomes, n_ranges, P, flags, max_locs)


def test_many_chunks_and_pair_arrays_that_grow(mods, genomes, monkeypatch):
    pkg, eng, synth, torch = mods
    n_windows = int(_reference(eng, genomes, 3, 0, 0)[3][-1])
    monkeypatch.setenv("MCQ_BUILD_CHUNK_WINDOWS", "9000")
    assert n_windows // 9000 >= 4
    _check_equal(eng, genomes, 2, 3, 0, 0)
    monkeypatch.delenv("MCQ_BUILD_CHUNK_WINDOWS")
    monkeypatch.setenv("MCQ_BUILD_PART_CAP", "1000")
    _check_equal(eng, genomes, 2, 3, 0, 0)
    monkeypatch.setenv("MCQ_BUILD_CHUNK_WINDOWS", "9000")
    _check_equal(eng, genomes, 5, 8, eng.MCQ_BUILD_REMOVE_OVERPOPULATED, 3)


def test_rank_split_and_remove_ambiguous_work_on_a_range_table(mods, genomes):
    pkg, eng, synth, torch = mods
    gb, goff, species = genomes
    rb = eng.RangeBuild(gb.data_ptr(), goff.data_ptr(), goff.numel() - 1, n_ranges=3, emulate_ranks=3, device=0)
    for t in rb:
        keys, off, locs, win = t.to_host()
        for r in range(3):
            part = t.rank_split(3, r)
            k2, o2, l2, w2 = part.to_host()
            ek, eo, el = _numpy_split(keys, off, locs, 3, r)
            assert np.array_equal(k2, ek) and np.array_equal(o2, eo) and np.array_equal(l2, el) and np.array_equal(w2, win)
            part.close()
        kept, removed = t.remove_ambiguous(species, max_keys=1)
        ek, eo, el, er = numpy_filter(keys, off, locs, species, 1)
        k2, o2, l2, _ = kept.to_host()
        assert removed == er and 0 < er < len(keys)
        assert np.array_equal(k2, ek) and np.array_equal(o2, eo) and np.array_equal(l2, el)
        assert np.array_equal(kept.tgt_windows(), t.tgt_windows())
        kept.close(); t.close()
    rb.close()


def test_ranges_without_features_are_empty_tables(mods):
    """64 ranges on 5 targets, and on one sequence of a single window (at most 16 features: most of the 64 ranges hold none)"""
    pkg, eng, synth, torch = mods
    dev = torch.device("cuda", 0)
    gb, goff, _ = synth.make_genomes(5, 1, 2000, 3000, 0.02, seed=12, device=dev)
    for bases, off in ((gb, goff), (gb[:100].contiguous(), torch.tensor([0, 100], dtype=torch.int64, device=dev))):
        nt = off.numel() - 1
        ref = eng.Table(bases.data_ptr(), off.data_ptr(), nt, emulate_ranks=2, device=0)
        keys, loff, locs, win_off = ref.to_host()
        rb = eng.RangeBuild(bases.data_ptr(), off.data_ptr(), nt, n_ranges=64, emulate_ranks=2, device=0)
        tables, n_empty = [], 0
        for t in rb:
            k, o, l, w = t.to_host()
            if t.n_keys == 0:
                n_empty += 1
                assert t.n_locs == 0 and np.array_equal(o, np.zeros(1, np.uint64)) and np.array_equal(w, win_off)
                assert t.shard_records(2, 0).shape == (0,) and t.rank_split(2, 0).n_keys == 0
            tables.append((k, o, l))
            t.close()
        assert len(tables) == 64 and (nt > 1 or n_empty >= 48)
        k2, o2, l2 = _sorted_union(tables)
        assert np.array_equal(k2, keys) and np.array_equal(o2, loff) and np.array_equal(l2, locs)
        rb.close(); ref.close()


def test_arguments_the_library_refuses(mods, genomes):
    pkg, eng, synth, torch = mods
    gb, goff, _ = genomes
    with pytest.raises(eng.McqError) as e:
        eng.RangeBuild(gb.data_ptr(), goff.data_ptr(), goff.numel() - 1, n_ranges=(1 << 20) + 1, device=0)
    assert e.value.code == eng.MCQ_E_UNSUPPORTED
    with pytest.raises(eng.McqError) as e:
        eng.RangeBuild(gb.data_ptr(), goff.data_ptr(), 0, n_ranges=1, device=0)
    assert e.value.code == eng.MCQ_E_ARG
    rb = eng.RangeBuild(gb.data_ptr(), goff.data_ptr(), goff.numel() - 1, n_ranges=0, device=0)      # from the free memory: one range here
    assert rb.n_ranges == 1
    rb.close()
