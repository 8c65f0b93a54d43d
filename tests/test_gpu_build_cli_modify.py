"""mcq_build_cli -modify on the GPU: a database built from the first records of a fixture's genomes and extended by the rest,
against the files the reference's own `mpiexec -n P metacache_mpi build` wrote for all of them (tests/golden/*/P*/*.db_<r>): in
the reference a bucket is appended to, so a database built from A and extended by B holds what one built from A and B holds when
B's targets get the later ids.  Then mcq_query_cli on the extended database, names that are taken, -out, and the options -modify
refuses."""
import gzip
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import build_inputs as bi
from golden_util import Fixture
from test_gpu_build_cli import _one_rank, mods        # noqa: F401  (mods is a fixture)
from test_gpu_cli import VARIANTS

pytestmark = pytest.mark.gpu
CASES = [(tag, P) for tag, (Ps, _) in sorted(bi.FIXTURES.items()) if bi.has_build_inputs(tag) for P in Ps]
NO_TAXONOMY = "tie"           # the fixture whose second run gets no -taxonomy: the taxa above the sequences are carried over


def _run(pkg, work, args, timeout=600):
    """a fresh child process: mcq_build_cli <args> in `work`"""
    return subprocess.run([pkg.build_cli_path()] + [str(a) for a in args], cwd=work, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True, timeout=timeout)


def _records(work):
    with open(os.path.join(work, "genomes", "all.fna"), "rb") as f:
        return [b">" + r for r in f.read().split(b">")[1:]]


def _lay_out(tag, work, more_b=()):
    """bi.lay_out, and the records of genomes/all.fna cut in order into genomes_a/a.fna (the first three fifths) and genomes_b/b.fna
    (the rest, then the records `more_b` picks from all of them): -> (records in a, records in all)"""
    bi.lay_out(tag, work)
    recs = _records(work)
    n_a = len(recs) * 3 // 5
    for name, part in (("a", recs[:n_a]), ("b", recs[n_a:] + [recs[i] for i in more_b])):
        os.makedirs(os.path.join(work, "genomes_" + name))
        with open(os.path.join(work, "genomes_" + name, name + ".fna"), "wb") as f:
            f.write(b"".join(part))
    return n_a, len(recs)


def _files(work, name, P):
    return [open(os.path.join(work, "%s.db_%d" % (name, r)), "rb").read() for r in range(P)]


_made = {}


@pytest.fixture(scope="module")
def two_runs(mods, tmp_path_factory):
    """(tag, P) -> (work directory, records in a, records in all, stdout of the second run): `mcq_build_cli tag P genomes_a
    -taxonomy tax`, then `mcq_build_cli tag P genomes_b -modify` with the fixture's options; made once, never written to again"""
    pkg = mods[0]

    def make(tag, P):
        if (tag, P) not in _made:
            work = str(tmp_path_factory.mktemp("%s_%d" % (tag, P)) / "w")
            n_a, n = _lay_out(tag, work)
            r = _run(pkg, work, [tag, P, "genomes_a", "-taxonomy", "tax"])
            assert r.returncode == 0, r.stderr[-2000:]
            first = _files(work, tag, P)
            r = _run(pkg, work, [tag, P, "genomes_b", "-modify"] + ([] if tag == NO_TAXONOMY else ["-taxonomy", "tax"]) + bi.FIXTURES[tag][1])
            assert r.returncode == 0, r.stderr[-2000:]
            assert _files(work, tag, P) != first and not [f for f in os.listdir(work) if f.endswith(".tmp")]
            _made[(tag, P)] = (work, n_a, n, r.stdout)
        return _made[(tag, P)]
    return make


@pytest.mark.parametrize("tag,P", CASES)
def test_built_from_a_and_extended_by_b_holds_what_the_references_build_of_both_holds(mods, two_runs, tag, P, tmp_path):
    """every rank's file against the golden one, as tests/test_gpu_build_cli.py compares a build: triples, mcq_refdb_info, key and
    location counts, taxon list -- but for the source of the sequence-level taxa, which names the two files as they were given,
    with indices from 1 in each -- and mcq_refdb_tgt_windows over all ranks.  overpop gets -remove-overpopulated-features in the
    second run only; tie gets no -taxonomy there"""
    pkg, eng, host = mods
    assert {t for t, _ in CASES} >= {"mini", "tie", "overpop", "noanc", "wide"} and (tag != "mini" or P in (2, 4, 8)) and NO_TAXONOMY in {t for t, _ in CASES}
    fx = Fixture(tag, P)
    work, n_a, n, stdout = two_runs(tag, P)
    assert 0 < n_a < n and (P < 8 or n_a < P or tag != "mini")          # mini at P = 8: ranks 6 and 7 own no old target
    assert ("%d sequences added to %d, 0 skipped" % (n - n_a, n_a)) in stdout
    for rank in range(P):
        mine = _one_rank(host, os.path.join(work, "%s.db_%d" % (tag, rank)), str(tmp_path), "mine%d" % rank)
        gold = _one_rank(host, fx.shard_paths[rank], str(tmp_path), "gold%d" % rank)
        assert mine[0] == gold[0], rank
        want = []
        for rec in gold[1]:
            rec = dict(rec)
            if rec["id"] < 0:
                t = -rec["id"] - 1
                assert rec["source"][:2] == ("genomes/all.fna", t + 1)
                rec["source"] = (("genomes_a/a.fna", t + 1) if t < n_a else ("genomes_b/b.fna", t - n_a + 1)) + rec["source"][2:]
            want.append(rec)
        assert mine[1] == want, rank
        assert mine[2] == gold[2], rank
        assert mine[3].shape == gold[3].shape and np.array_equal(mine[3], gold[3]), rank
    a = host.RefDb(os.path.join(work, tag), P, meta_only=True)
    b = host.RefDb(fx.shard_paths[0][: -len(".db_0")], P, meta_only=True)
    assert np.array_equal(a.tgt_windows(), b.tgt_windows())


def test_query_cli_on_the_extended_database_writes_the_references_out_file(mods, two_runs, tmp_path):
    """mcq_query_cli on the extended mini at P = 4 with the option sets of tests/test_gpu_cli.py: the -out file the reference wrote
    on its own database of all genomes (cli_*.out.gz), compared as there -- sorted, "# time:" / "# speed:" masked"""
    pkg, eng, host = mods
    tag, P = "mini", 4
    fx = Fixture(tag, P)
    work = str(tmp_path / "w")
    shutil.copytree(two_runs(tag, P)[0], work)
    for fn, seqs in (("r1.fq", fx.r1), ("r2.fq", fx.r2)):
        with open(os.path.join(work, fn), "w") as f:
            for n, s in zip(fx.names, seqs):
                f.write("@%s\n%s\n+\n%s\n" % (n, s, "I" * len(s)))

    def norm(text):
        text = re.sub(r"^# time:    .*$", "# time:    T ms", text, flags=re.M)
        text = re.sub(r"^# speed:   .*$", "# speed:   S queries/min", text, flags=re.M)
        return sorted(text.split("\n"))
    for variant in sorted(VARIANTS):
        q = subprocess.run([pkg.cli_path(), tag, str(P), "r1.fq", "r2.fq", "-lowest", fx.q["lowest"], "-maxcand", str(fx.maxcand),
                            "-hitmin", str(fx.hitmin), "-hitdiff", str(fx.q["hitdiff"]), "-threads", "2", "-out", "out_%s.txt" % variant] + VARIANTS[variant],
                           cwd=work, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        assert q.returncode == 0, (variant, q.stderr[-2000:])
        with gzip.open(os.path.join(os.path.dirname(fx.shard_paths[0]), "cli_%s.out.gz" % variant), "rt") as f:
            ref = f.read()
        assert norm(open(os.path.join(work, "out_%s.txt" % variant)).read()) == norm(ref), variant


def test_names_that_are_taken_are_skipped_and_counted(mods, two_runs, tmp_path):
    """genomes_b ends with a record of genomes_a and with one of its own, twice: none of the three becomes a target, the first
    line on stdout says so, and the files are those of the run without them, byte for byte"""
    pkg, eng, host = mods
    tag, P = "mini", 4
    plain, n_a, n, _ = two_runs(tag, P)
    work = str(tmp_path / "w")
    assert _lay_out(tag, work, more_b=(1, n_a + 1, n_a + 1)) == (n_a, n)
    r = _run(pkg, work, [tag, P, "genomes_a", "-taxonomy", "tax"])
    assert r.returncode == 0, r.stderr[-2000:]
    r = _run(pkg, work, [tag, P, "genomes_b", "-modify", "-taxonomy", "tax"])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().split("\n")
    assert lines[0].startswith("%d sequences added to %d, 3 skipped" % (n - n_a, n_a)), r.stdout
    assert lines[-1].startswith("%d targets, " % n), r.stdout
    assert _files(work, tag, P) == _files(plain, tag, P)


def _built_from_a(pkg, tmp_path, tag="mini", P=4):
    work = str(tmp_path / "w")
    _lay_out(tag, work)
    r = _run(pkg, work, [tag, P, "genomes_a", "-taxonomy", "tax"])
    assert r.returncode == 0, r.stderr[-2000:]
    return work, _files(work, tag, P)


def test_out_writes_a_second_database_and_leaves_the_first(mods, two_runs, tmp_path):
    pkg, eng, host = mods
    work, first = _built_from_a(pkg, tmp_path)
    r = _run(pkg, work, ["mini", 4, "genomes_b", "-modify", "-taxonomy", "tax", "-out", "grown"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert _files(work, "mini", 4) == first
    assert _files(work, "grown", 4) == _files(two_runs("mini", 4)[0], "mini", 4)
    assert "grown.db_0 .. _3" in r.stdout
    r = _run(pkg, work, ["other", 4, "genomes_b", "-taxonomy", "tax", "-out", "grown2"])
    assert r.returncode != 0 and "ABORT: -out NEWDB goes with -modify" in r.stderr and not [f for f in os.listdir(work) if f.startswith(("other", "grown2"))]


def test_another_sketch_parameter_and_an_unknown_option_end_the_run_and_leave_the_database(mods, two_runs, tmp_path):
    """-kmerlen 15 on a database of k = 16: non-zero, an ABORT line with the option and the database's value, the files untouched
    and no temporary file left (a divergence: the reference goes on with the database's k in silence); the database's own values
    pass; -no-such-option still aborts"""
    pkg, eng, host = mods
    work, first = _built_from_a(pkg, tmp_path)
    before = sorted(os.listdir(work))
    for extra, words in ((["-kmerlen", "15"], ("-kmerlen 15", "16")), (["-winstride", "100"], ("-winstride 100", "113")),
                         (["-sketchlen", "8"], ("-sketchlen 8", "16")), (["-winlen", "127"], ("-winlen 127", "128"))):
        r = _run(pkg, work, ["mini", 4, "genomes_b", "-modify"] + extra)
        abort = [l for l in r.stderr.split("\n") if l.startswith("ABORT:")]
        assert r.returncode != 0 and len(abort) == 1 and all(w in abort[0] for w in words), (extra, r.returncode, r.stderr[-500:])
        assert _files(work, "mini", 4) == first and sorted(os.listdir(work)) == before
    r = _run(pkg, work, ["mini", 4, "genomes_b", "-modify", "-no-such-option"])
    assert r.returncode != 0 and "ABORT: unknown option" in r.stderr
    assert _files(work, "mini", 4) == first and sorted(os.listdir(work)) == before
    r = _run(pkg, work, ["absent", 4, "genomes_b", "-modify"])
    assert r.returncode != 0 and "ABORT:" in r.stderr and sorted(os.listdir(work)) == before
    r = _run(pkg, work, ["mini", 4, "genomes_b", "-modify", "-kmerlen", "16", "-sketchlen", "16", "-winlen", "128", "-winstride", "113"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert _files(work, "mini", 4) == _files(two_runs("mini", 4)[0], "mini", 4)
