"""The host inputs of mcq_build_cli -modify (no GPU): the genome reader opened after an existing database
(mcq_genome_reader_open_after) and the database's taxon records as records to write (mcq_refdb_taxa), on the golden shard files the
reference built for mini at P = 2."""
import importlib

import numpy as np
import pytest

import build_inputs as bi
from golden_util import Fixture


@pytest.fixture(scope="module")
def host():
    pkg = importlib.import_module("metacache-mpi_amd")
    pkg.build_host()
    return importlib.import_module("metacache-mpi_amd.host")


@pytest.fixture(scope="module")
def mini(host):
    fx = Fixture("mini", 2)
    prefix = fx.shard_paths[0][: -len(".db_0")]
    return host.RefDb(prefix, 2, meta_only=True), host.RefDb(prefix, 2)


def _fasta(records):
    return b"".join(b">%s\n%s\n" % (h, s) for h, s in records)


def test_ids_go_on_behind_the_databases_and_its_names_are_taken(host, mini, tmp_path):
    """two files of new records among which stand two names of the database, and one new name twice: the reader gives the new
    ones the ids n_old, n_old + 1, ... in reading order (a skipped record takes no id but counts in its file's index), as the Python
    restatement of the reference's reader does when the database's names are taken beforehand; both openers of the database serve"""
    meta, full = mini
    n_old = meta.info.n_targets
    assert n_old == 10
    old_names = [meta.taxon_name(k) for k in range(meta.info.n_taxa) if meta.taxon_rank(k) == host.RANK_SEQUENCE]
    assert len(old_names) == n_old and "NC_000003.1 taxid" in old_names
    files = [("x.fna", [(b"NC_900001.1 taxid|101 new", b"ACGT" * 40), (b"NC_000003.1 taxid|102 in the database", b"TTGCA" * 30),
                        (b"NC_900002.1 new, no taxid", b"GATTACA" * 20), (b"NC_900001.1 taxid|5 again", b"CC" * 50)]),
             ("y.fna", [(b"NC_000010.1 taxid|301 in the database", b"A" * 90), (b"NC_900003.1 taxid|202 new", b"GGA" * 50)])]
    paths = []
    for name, recs in files:
        paths.append(str(tmp_path / name))
        with open(paths[-1], "wb") as f:
            f.write(_fasta(recs))
    want = bi.read_genomes([(p, _fasta(r)) for p, (_, r) in zip(paths, files)])      # (without a database: five targets)
    taken = {n.encode() for n in old_names}
    seen, expect = set(taken), []
    for p, (_, recs) in zip(paths, files):
        for i, (h, s) in enumerate(recs):
            name = bi.target_name(h)
            if name in seen:
                continue
            seen.add(name)
            expect.append((name, bi.parent_taxid(h), p, i + 1, s))
    assert [e[0] for e in expect] == [b"NC_900001.1 taxid", b"NC_900002.1", b"NC_900003.1 taxid"] and len(want) == 5
    for db in (meta, full):
        for cap, io_bytes in ((1 << 16, 1 << 20), (7, 5)):
            skipped = []
            bases, recs, lens, _ = host.read_genomes(paths, cap, io_bytes, after=db, skipped=skipped)
            assert skipped == [3]
            assert bases == b"".join(e[4] for e in expect) and lens == [len(e[4]) for e in expect]
            for i, (r, e) in enumerate(zip(recs, expect)):
                assert (r["id"], r["parent"], r["rank"], r["name"].encode(), r["file"], r["index"], r["windows"]) == \
                       (-(n_old + i + 1), e[1], host.RANK_SEQUENCE, e[0], e[2], e[3], 0)
    # the plain opener is what it was: ids from -1, only the repeat inside the run is skipped
    skipped = []
    _, recs, _, _ = host.read_genomes(paths, 1 << 16, skipped=skipped)
    assert [r["id"] for r in recs] == [-1, -2, -3, -4, -5] and skipped == [1]
    assert [(r["name"].encode(), r["index"]) for r in recs] == [(w[0], w[3]) for w in want]


def test_the_databases_taxon_records_come_back_as_the_files_hold_them(host, mini, tmp_path):
    """mcq_refdb_taxa against the accessors, record by record in file order; written to a file of their own and read back they are
    the taxon list of rank 0's golden file, its `windows` included"""
    meta, full = mini
    for db in (meta, full):
        taxa = db.taxa()
        assert len(taxa) == db.info.n_taxa > db.info.n_targets
        assert [dict(id=t["id"], parent=t["parent"], rank=t["rank"], name=t["name"], source=(t["file"], t["index"], t["windows"]))
                for t in taxa] == bi.taxon_list(db)
    taxa = meta.taxa()
    windows = meta.tgt_windows()
    for t in taxa:                               # rank 0 of 2 owns the even targets: only their windows are in its file
        if t["id"] < 0:
            tgt = -t["id"] - 1
            assert t["windows"] == (int(windows[tgt]) if tgt % 2 == 0 else 0)
    fx = Fixture("mini", 2)
    p = fx.params
    host.write_shard(str(tmp_path / "again.db_0"), dict(k=p["k"], sketch_size=p["s"], winlen=p["winlen"], winstride=p["winstride"], q_k=p["qk"],
                                                        q_sketch_size=p["qs"], q_winlen=p["qwinlen"], q_winstride=p["qwinstride"],
                                                        max_locs_per_feature=p["maxlocs"]),
                     taxa, meta.info.n_targets, np.zeros(0, np.uint32), np.zeros(1, np.uint64), np.zeros(0, np.uint64))
    again = host.RefDb(str(tmp_path / "again"), 1)
    assert bi.taxon_list(again) == bi.taxon_list(full) and again.taxa() == taxa
