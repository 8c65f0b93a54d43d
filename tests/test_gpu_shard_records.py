"""mcq_table_shard_records: one reference rank's key records of a table, made on the GPU as the bytes of its shard file, against
the numpy serializer (tests/shard_records_ref.py, itself checked against mcq_refdb_write_shard's bytes in
tests/test_host_shard_writer.py) of the numpy rank filter of the table.  Everything is an equality."""
import importlib

import numpy as np
import pytest

from shard_records_ref import serialize
from test_gpu_build_cli import _numpy_split

pytestmark = pytest.mark.gpu
GUARD = 4096


@pytest.fixture(scope="module")
def mods():
    import torch
    pkg = importlib.import_module("metacache-mpi_amd")
    return pkg, importlib.import_module("metacache-mpi_amd.engine"), importlib.import_module("metacache-mpi_amd.synth"), torch


@pytest.fixture(scope="module")
def genomes(mods):
    pkg, eng, synth, torch = mods
    gb, goff, _ = synth.make_genomes(300, 10, 2000, 3000, 0.02, seed=11, device=torch.device("cuda", 0))
    assert goff.numel() - 1 == 3000
    return gb, goff


def _check_rank(table, host_arrays, P, r):
    """the records of rank r and the three sizes, against the serializer of the numpy filter; returns the rank's list lengths"""
    keys, off, locs = host_arrays
    ek, eo, el = _numpy_split(keys, off, locs, P, r)
    want, n_keys, n_locs = serialize(ek, eo, el)
    assert table.shard_records_into(P, r, None, 0) == (len(want), n_keys, n_locs), (P, r)
    got = table.shard_records(P, r)
    assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want), (P, r)
    return np.diff(eo.astype(np.int64))


@pytest.mark.parametrize("P", [1, 2, 3, 8, 64])
def test_every_ranks_records_equal_the_serialized_numpy_filter(mods, genomes, P):
    pkg, eng, synth, torch = mods
    gb, goff = genomes
    table = eng.Table(gb.data_ptr(), goff.data_ptr(), goff.numel() - 1, emulate_ranks=P, device=0)
    host_arrays = table.to_host()[:3]
    assert table.n_keys > 100000
    total = 0
    for r in range(P):
        total += int(_check_rank(table, host_arrays, P, r).sum())
    assert total == table.n_locs
    table.close()


def test_a_key_count_that_is_no_multiple_of_four(mods, genomes):
    """four keys per wave: the last wave of a table whose key count is not a multiple of 4 has groups without a key.  The union table's
    count is what the data gives, so the table is taken from it and its rank splits: the first whose count is not a multiple."""
    pkg, eng, synth, torch = mods
    gb, goff = genomes
    union = eng.Table(gb.data_ptr(), goff.data_ptr(), goff.numel() - 1, emulate_ranks=3, device=0)
    tables = [union] + [union.rank_split(3, r) for r in range(3)] + [union.rank_split(2, r) for r in range(2)]
    odd = [t for t in tables if t.n_keys % 4]
    assert odd, [t.n_keys for t in tables]
    t = odd[0]
    host_arrays = t.to_host()[:3]
    for r in range(3):
        _check_rank(t, host_arrays, 3, r)
    for x in tables:
        x.close()


def test_five_targets_at_eight_ranks(mods):
    """ranks 5..7 own nothing: 0 bytes, not an error; rank >= n_ranks is MCQ_E_ARG"""
    pkg, eng, synth, torch = mods
    gb, goff, _ = synth.make_genomes(5, 1, 2000, 3000, 0.02, seed=12, device=torch.device("cuda", 0))
    table = eng.Table(gb.data_ptr(), goff.data_ptr(), 5, emulate_ranks=8, device=0)
    host_arrays = table.to_host()[:3]
    for r in range(8):
        lens = _check_rank(table, host_arrays, 8, r)
        assert (len(lens) > 0) == (r < 5)
    for r in (5, 6, 7):
        assert table.shard_records_into(8, r, None, 0) == (0, 0, 0) and table.shard_records(8, r).shape == (0,)
    for P, r in ((8, 8), (8, 9), (1, 1), (0, 0)):
        with pytest.raises(eng.McqError) as e:
            table.shard_records_into(P, r, None, 0)
        assert e.value.code == eng.MCQ_E_ARG
    table.close()


def _copies_table(mods, P):
    """Lists at the boundaries of the 16-lane groups: distinct random 2 kb sequences, copied so that every rank of P gets 1, 15, 16, 17
    and 260 copies of one of them (260 > 254: the build's limit cuts that list to 254), behind 40 random sequences of their own"""
    pkg, eng, synth, torch = mods
    rng = np.random.default_rng(5)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    seqs = [acgt[rng.integers(0, 4, 2000)] for _ in range(40)]
    for per_rank in (1, 15, 16, 17, 260):
        one = acgt[rng.integers(0, 4, 2000)]
        seqs += [one] * (per_rank * P)           # consecutive target ids: per_rank of them on every rank
    off = np.zeros(len(seqs) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    dev = torch.device("cuda", 0)
    gb, goff = torch.from_numpy(np.concatenate(seqs)).to(dev), torch.from_numpy(off).to(dev)
    table = eng.Table(gb.data_ptr(), goff.data_ptr(), len(seqs), emulate_ranks=P, device=0)
    torch.cuda.synchronize()
    return table


@pytest.mark.parametrize("P", [1, 2])
def test_lists_at_the_group_boundaries(mods, P):
    pkg, eng, synth, torch = mods
    table = _copies_table(mods, P)
    host_arrays = table.to_host()[:3]
    for r in range(P):
        lens = set(_check_rank(table, host_arrays, P, r).tolist())
        assert {1, 15, 16, 17, 254} <= lens and max(lens) == 254, (P, r, sorted(lens))
    table.close()


def test_capacity_sizes_and_the_guard_behind_the_buffer(mods):
    """cap_bytes = n_bytes - 1: MCQ_E_CAPACITY and nothing written; cap_bytes = n_bytes: the records, and the bytes behind them
    stay what they were"""
    pkg, eng, synth, torch = mods
    table = _copies_table(mods, 2)
    keys, off, locs = table.to_host()[:3]
    want, n_keys, n_locs = serialize(*_numpy_split(keys, off, locs, 2, 1))
    n_bytes = len(want)
    assert table.shard_records_into(2, 1, None, 0) == (n_bytes, n_keys, n_locs) and n_bytes > 0
    buf = torch.full((n_bytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    with pytest.raises(eng.McqError) as e:
        table.shard_records_into(2, 1, buf.data_ptr(), n_bytes - 1)
    assert e.value.code == eng.MCQ_E_CAPACITY
    assert bool((buf == 0xA5).all())
    assert table.shard_records_into(2, 1, buf.data_ptr(), n_bytes) == (n_bytes, n_keys, n_locs)
    got = buf.cpu().numpy()
    assert np.array_equal(got[:n_bytes], want) and (got[n_bytes:] == 0xA5).all()
    table.close()


def test_an_empty_table(mods):
    """a table without keys (the rank split of a rank that owns nothing) gives 0 bytes at every rank, with and without a buffer"""
    pkg, eng, synth, torch = mods
    gb, goff, _ = synth.make_genomes(5, 1, 2000, 3000, 0.02, seed=12, device=torch.device("cuda", 0))
    table = eng.Table(gb.data_ptr(), goff.data_ptr(), 5, emulate_ranks=8, device=0)
    empty = table.rank_split(8, 7)
    assert empty.n_keys == 0
    buf = torch.full((GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
    for P, r in ((1, 0), (8, 0), (8, 7)):
        assert empty.shard_records_into(P, r, None, 0) == (0, 0, 0)
        assert empty.shard_records_into(P, r, buf.data_ptr(), GUARD) == (0, 0, 0)
        assert empty.shard_records(P, r).shape == (0,)
    assert bool((buf == 0xA5).all())
    empty.close(); table.close()
