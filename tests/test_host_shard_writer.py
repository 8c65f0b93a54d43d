"""mcq_shard_writer_* (include/mcq_host.h): a shard file written in blocks of key records is the file mcq_refdb_write_shard writes
at once; and the numpy serializer of the records (tests/shard_records_ref.py), which the GPU tests of mcq_table_shard_records use
as their reference, is checked here against that function's own bytes."""
import filecmp
import importlib
import os
import struct

import numpy as np
import pytest

from golden_util import Fixture
from shard_records_ref import serialize

CASES = [("mini", 2), ("tie", 2)]


@pytest.fixture(scope="module")
def host():
    pkg = importlib.import_module("metacache-mpi_amd")
    pkg.build_host()
    return importlib.import_module("metacache-mpi_amd.host")


def _params(fx):
    p = fx.params
    return dict(k=p["k"], sketch_size=p["s"], winlen=p["winlen"], winstride=p["winstride"], q_k=p["qk"], q_sketch_size=p["qs"],
                q_winlen=p["qwinlen"], q_winstride=p["qwinstride"], max_locs_per_feature=p["maxlocs"])


def _golden_shards(host, tag, P, tmp):
    """every golden shard of the fixture through host.RefDb, alone: (rank, taxa, n_targets, keys, list_off, locs)"""
    fx = Fixture(tag, P)
    for r, path in enumerate(fx.shard_paths):
        d = os.path.join(tmp, "in_%s_%d" % (tag, r))
        os.makedirs(d)
        os.symlink(os.path.abspath(path), os.path.join(d, "x.db_0"))
        db = host.RefDb(os.path.join(d, "x"), 1)
        keys, off, locs = db.table()
        yield fx, r, db.taxa(), db.info.n_targets, keys, off, locs
        db.close()


@pytest.mark.parametrize("tag,P", CASES)
def test_the_numpy_serializer_equals_the_tail_of_the_written_file(host, tag, P, tmp_path):
    n = 0
    for fx, r, taxa, nt, keys, off, locs in _golden_shards(host, tag, P, str(tmp_path)):
        whole = str(tmp_path / ("whole_%d" % r))
        host.write_shard(whole, _params(fx), taxa, nt, keys, off, locs)
        data = open(whole, "rb").read()
        rec, n_keys, n_locs = serialize(keys, off, locs)
        assert n_keys == len(keys) > 0 and n_locs == len(locs) and len(rec) == 21 * n_keys + 8 * n_locs
        assert data[len(data) - len(rec):] == rec.tobytes(), r
        assert data[len(data) - len(rec) - 16:len(data) - len(rec)] == struct.pack("<QQ", n_keys, n_locs), r
        n += 1
    assert n == P


def _blocks(keys, off, locs, n_blocks):
    """the records cut into n_blocks runs of whole keys, an empty block in the middle of them (n_blocks > 1)"""
    cuts = np.linspace(0, len(keys), n_blocks + 1).astype(int)
    out = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        lo, hi = int(off[a]), int(off[b])
        out.append(serialize(keys[a:b], off[a:b + 1] - off[a], locs[lo:hi]))
    if n_blocks > 1:
        out.insert(n_blocks // 2, (np.zeros(0, np.uint8), 0, 0))
    return out


@pytest.mark.parametrize("tag,P", CASES)
@pytest.mark.parametrize("n_blocks", [1, 2, 7])
def test_a_file_written_in_blocks_is_the_file_written_at_once(host, tag, P, n_blocks, tmp_path):
    for fx, r, taxa, nt, keys, off, locs in _golden_shards(host, tag, P, str(tmp_path)):
        whole, blocks = str(tmp_path / ("whole_%d" % r)), str(tmp_path / ("blocks_%d" % r))
        host.write_shard(whole, _params(fx), taxa, nt, keys, off, locs)
        w = host.ShardWriter(blocks, _params(fx), taxa, nt)
        parts = _blocks(keys, off, locs, n_blocks)
        assert len(parts) == n_blocks + (n_blocks > 1) and sum(k for _, k, _ in parts) == len(keys)
        for rec, n_keys, n_locs in parts:
            w.append(rec, n_keys, n_locs)
        w.close()
        assert filecmp.cmp(whole, blocks, shallow=False), r


def test_a_file_without_keys_opens(host, tmp_path):
    fx = Fixture("mini", 2)
    fx, r, taxa, nt, keys, off, locs = next(_golden_shards(host, "mini", 2, str(tmp_path)))
    w = host.ShardWriter(str(tmp_path / "empty.db_0"), _params(fx), taxa, nt)
    w.append(np.zeros(0, np.uint8), 0, 0)
    w.close()
    whole = str(tmp_path / "whole.db_0")
    host.write_shard(whole, _params(fx), taxa, nt, np.zeros(0, np.uint32), np.zeros(1, np.uint64), np.zeros(0, np.uint64))
    assert filecmp.cmp(whole, str(tmp_path / "empty.db_0"), shallow=False)
    meta = host.RefDb(str(tmp_path / "empty"), 1, meta_only=True)
    assert meta.info.n_targets == nt and meta.info.n_taxa == len(taxa) and meta.file_stats(0)[1:] == (0, 0)
    assert list(meta.stream(0)) == []


def test_a_path_that_cannot_be_opened_and_a_block_of_the_wrong_size_fail_with_a_message(host, tmp_path):
    fx, r, taxa, nt, keys, off, locs = next(_golden_shards(host, "mini", 2, str(tmp_path)))
    with pytest.raises(RuntimeError, match="can't open file .*no_such_dir"):
        host.ShardWriter(str(tmp_path / "no_such_dir" / "x.db_0"), _params(fx), taxa, nt)
    w = host.ShardWriter(str(tmp_path / "x.db_0"), _params(fx), taxa, nt)
    with pytest.raises(RuntimeError, match="21 n_keys"):
        w.append(np.zeros(30, np.uint8), 1, 1)
    w.close()


def test_a_write_error_is_reported(host, tmp_path):
    """a file on a full device (a link to /dev/full): open may succeed, the error comes out by close() at the latest"""
    fx, r, taxa, nt, keys, off, locs = next(_golden_shards(host, "mini", 2, str(tmp_path)))
    os.symlink("/dev/full", str(tmp_path / "full.db_0"))
    rec, n_keys, n_locs = serialize(keys, off, locs)
    with pytest.raises(RuntimeError, match="write error on .*full.db_0"):
        w = host.ShardWriter(str(tmp_path / "full.db_0"), _params(fx), taxa, nt)
        w.append(rec, n_keys, n_locs)
        w.close()
