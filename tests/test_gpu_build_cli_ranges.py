"""mcq_build_cli -ranges N: the build in feature-hash ranges, a fresh child process per build as tests/test_gpu_build_cli.py starts
it.  The files must hold what the reference's hold (compared by content, as there) and what the one-piece route writes; with one
range they are the same bytes."""
import filecmp
import gzip
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import build_inputs as bi
from golden_util import Fixture
from test_gpu_build_cli import CASES, _build, _one_rank
from test_gpu_cli import VARIANTS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    pkg = importlib.import_module("metacache-mpi_amd")
    pkg.build_host()
    return pkg, importlib.import_module("metacache-mpi_amd.engine"), importlib.import_module("metacache-mpi_amd.host")


def _db_files(work, name):
    return sorted(f for f in os.listdir(work) if f.startswith(name + ".db"))


@pytest.mark.parametrize("tag,P", CASES)
def test_files_of_three_ranges_hold_what_the_references_hold(mods, tag, P, tmp_path):
    """every rank's file of a -ranges 3 build against the golden one, as test_shard_files_hold_what_the_references_hold compares the
    one-piece build's: parameters, taxon list with the rank's `windows`, key and location counts, the sorted triples; no temporary
    file is left"""
    pkg, eng, host = mods
    assert {t for t, _ in CASES} >= {"mini", "tie", "overpop", "noanc", "wide"} and {P_ for t, P_ in CASES if t == "mini"} >= {2, 4, 8}
    fx = Fixture(tag, P)
    work = bi.lay_out(tag, str(tmp_path / "w"))
    r = _build(pkg, work, tag, P, bi.FIXTURES[tag][1] + ["-ranges", "3"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert _db_files(work, tag) == sorted("%s.db_%d" % (tag, rank) for rank in range(P))
    for rank in range(P):
        mine = _one_rank(host, os.path.join(work, "%s.db_%d" % (tag, rank)), str(tmp_path), "mine%d" % rank)
        gold = _one_rank(host, fx.shard_paths[rank], str(tmp_path), "gold%d" % rank)
        assert mine[0] == gold[0], rank
        assert mine[1] == gold[1], rank
        assert mine[2] == gold[2], rank
        assert mine[3].shape == gold[3].shape and np.array_equal(mine[3], gold[3]), rank
    a = host.RefDb(os.path.join(work, tag), P, meta_only=True)
    b = host.RefDb(fx.shard_paths[0][: -len(".db_0")], P, meta_only=True)
    assert np.array_equal(a.tgt_windows(), b.tgt_windows())


@pytest.mark.parametrize("tag,P", [("mini", 4), ("overpop", 2)])
def test_one_range_writes_the_bytes_of_the_default_run(mods, tag, P, tmp_path):
    """-ranges 1 against a run without the option: the P files are the same bytes; -ranges 3: files of the same size (the same
    records in another order); the summary line is the default run's, and names the ranges under MCQ_BUILD_TRACE"""
    pkg, eng, host = mods
    work = bi.lay_out(tag, str(tmp_path / "w"))
    runs = {}
    for name, extra in (("plain", []), ("one", ["-ranges", "1"]), ("three", ["-ranges", "3"])):
        runs[name] = _build(pkg, work, name, P, bi.FIXTURES[tag][1] + extra)
        assert runs[name].returncode == 0, runs[name].stderr[-2000:]
    for rank in range(P):
        paths = {n: os.path.join(work, "%s.db_%d" % (n, rank)) for n in runs}
        assert filecmp.cmp(paths["plain"], paths["one"], shallow=False), rank
        assert os.path.getsize(paths["three"]) == os.path.getsize(paths["plain"]), rank
    for name in ("one", "three"):
        assert runs[name].stdout.replace(name + ".db", "plain.db") == runs["plain"].stdout
    env = dict(os.environ, MCQ_BUILD_TRACE="1")
    t = subprocess.run([pkg.build_cli_path(), "traced", str(P), "genomes", "-taxonomy", "tax"] + bi.FIXTURES[tag][1] + ["-ranges", "3"], cwd=work,
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert t.returncode == 0 and t.stdout.replace("traced.db", "plain.db") == runs["plain"].stdout.rstrip("\n") + " (3 ranges)\n"
    assert "-ranges" in subprocess.run([pkg.build_cli_path(), "-help"], stdout=subprocess.PIPE, text=True).stdout


def test_a_rank_without_targets_gets_a_file_the_host_library_opens(mods, tmp_path):
    """noanc (4 targets) at P = 8 in three ranges: ranks 4..7 own nothing; their files are written all the same and mcq_refdb_open
    reads all eight: the union is that of the golden P = 4 files"""
    pkg, eng, host = mods
    work = bi.lay_out("noanc", str(tmp_path / "w"))
    r = _build(pkg, work, "noanc", 8, ["-ranges", "3"])
    assert r.returncode == 0, r.stderr[-2000:]
    db = host.RefDb(os.path.join(work, "noanc"), 8)
    meta = host.RefDb(os.path.join(work, "noanc"), 8, meta_only=True)
    for rank in range(8):
        _, n_keys, n_locs = meta.file_stats(rank)
        assert (n_keys > 0 and n_locs > 0) if rank < 4 else (n_keys == 0 and n_locs == 0)
    gold = host.RefDb(Fixture("noanc", 4).shard_paths[0][: -len(".db_0")], 4)
    for a, b in zip(db.table(), gold.table()):
        assert np.array_equal(a, b)


def test_remove_ambig_features_in_ranges_is_the_filter_of_the_whole_table(mods, tmp_path):
    """mini, P = 2, -remove-ambig-features species: the same triples and taxon lists with and without -ranges 3, and the same
    printed "N of M removed" (the counts of the ranges add up)"""
    pkg, eng, host = mods
    work = bi.lay_out("mini", str(tmp_path / "w"))
    opts = bi.FIXTURES["mini"][1] + ["-remove-ambig-features", "species"]
    whole = _build(pkg, work, "whole", 2, opts)
    parts = _build(pkg, work, "parts", 2, opts + ["-ranges", "3"])
    assert whole.returncode == 0 and parts.returncode == 0, (whole.stderr[-1000:], parts.stderr[-1000:])
    line = re.compile(r"^ambiguous features on rank species \(more than 1 taxa\): (\d+) of (\d+) removed$", re.M)
    assert line.search(whole.stdout) and line.search(whole.stdout).groups() == line.search(parts.stdout).groups()
    assert int(line.search(whole.stdout).group(1)) > 0
    assert parts.stdout.replace("parts.db", "whole.db") == whole.stdout
    for rank in range(2):
        a = _one_rank(host, os.path.join(work, "whole.db_%d" % rank), str(tmp_path), "whole%d" % rank)
        b = _one_rank(host, os.path.join(work, "parts.db_%d" % rank), str(tmp_path), "parts%d" % rank)
        assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2], rank
        assert a[3].shape == b[3].shape and np.array_equal(a[3], b[3]), rank


def test_query_cli_on_a_database_built_in_ranges_writes_the_references_out_file(mods, tmp_path):
    """mini, P = 4, built with -ranges 3, then mcq_query_cli: the -out file the reference wrote on its own database"""
    pkg, eng, host = mods
    tag, P, variant = "mini", 4, sorted(VARIANTS)[0]
    fx = Fixture(tag, P)
    work = bi.lay_out(tag, str(tmp_path / "w"))
    r = _build(pkg, work, tag, P, bi.FIXTURES[tag][1] + ["-ranges", "3"])
    assert r.returncode == 0, r.stderr[-2000:]
    for fn, seqs in (("r1.fq", fx.r1), ("r2.fq", fx.r2)):
        with open(os.path.join(work, fn), "w") as f:
            for n, s in zip(fx.names, seqs):
                f.write("@%s\n%s\n+\n%s\n" % (n, s, "I" * len(s)))

    def norm(text):
        text = re.sub(r"^# time:    .*$", "# time:    T ms", text, flags=re.M)
        text = re.sub(r"^# speed:   .*$", "# speed:   S queries/min", text, flags=re.M)
        return sorted(text.split("\n"))
    q = subprocess.run([pkg.cli_path(), tag, str(P), "r1.fq", "r2.fq", "-lowest", fx.q["lowest"], "-maxcand", str(fx.maxcand),
                        "-hitmin", str(fx.hitmin), "-hitdiff", str(fx.q["hitdiff"]), "-threads", "2", "-out", "out.txt"] + VARIANTS[variant],
                       cwd=work, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert q.returncode == 0, q.stderr[-2000:]
    with gzip.open(os.path.join(os.path.dirname(fx.shard_paths[0]), "cli_%s.out.gz" % variant), "rt") as f:
        ref = f.read()
    assert norm(open(os.path.join(work, "out.txt")).read()) == norm(ref)


def test_modify_in_ranges_is_refused_before_anything_is_read(mods, tmp_path):
    pkg, eng, host = mods
    work = bi.lay_out("mini", str(tmp_path / "w"))
    before = sorted(os.listdir(work))
    r = subprocess.run([pkg.build_cli_path(), "nothere", "2", "genomes", "-modify", "-ranges", "2"], cwd=work,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode != 0 and "ABORT:" in r.stderr and "-ranges" in r.stderr and "can't open" not in r.stderr
    assert sorted(os.listdir(work)) == before
    r = _build(pkg, work, "bad", 2, ["-ranges", "0"])
    assert r.returncode != 0 and "ABORT:" in r.stderr and sorted(os.listdir(work)) == before


def test_a_run_that_fails_leaves_no_file(mods, tmp_path):
    """a -ranges value the library refuses (more than 2^20), after the genomes were read; and a run whose second file stands on a
    full device (its temporary name is a link to /dev/full, made before the run): the records of the first range cannot be written,
    the run ends non-zero with ABORT:, and neither DB.db_* nor a temporary file is left"""
    pkg, eng, host = mods
    work = bi.lay_out("mini", str(tmp_path / "w"))
    before = sorted(os.listdir(work))
    r = _build(pkg, work, "refused", 2, ["-ranges", "2000000"])
    assert r.returncode != 0 and "ABORT:" in r.stderr and "too many ranges" in r.stderr, r.stderr[-500:]
    assert sorted(os.listdir(work)) == before
    os.symlink("/dev/full", os.path.join(work, "full.db_1.tmp"))
    r = _build(pkg, work, "full", 2, ["-ranges", "3"])
    assert r.returncode != 0 and "ABORT: write error on full.db_1.tmp" in r.stderr, r.stderr[-500:]
    assert sorted(os.listdir(work)) == before
