"""-exclude RANK, -ground-truth and -precision through mcq_query_cli.

The four -exclude runs are compared, byte for byte after sorting and with the measured values of "# time:" and "# speed:" taken
out, with the whole -out file the reference wrote for the same options and the same reads (tests/golden/*/P*/cli_excl_*.out.gz,
make_golden_evaluation.py; the reads are the fixture's under the headers of <tag>/eval_headers.json).  The reference's MPI program
forgets the truth before it evaluates, so it pins no truth column and no "ground truth" block: those are
checked against this file's own computation from eval_headers.json, nodes.dmp / names.dmp and the classifications of the same
output, with assign_known_correct and the summary templates as test_host_ground_truth.py restates them."""
import gzip
import importlib
import json
import os
import re
import shutil
import subprocess

import pytest

from golden_util import GOLDEN, Fixture
from test_host_ground_truth import RNONE, ROOT, _restated, _summary

pytestmark = pytest.mark.gpu

RUNS = {("mini", 4, "species"): ["-exclude", "species"],
        ("mini", 4, "genus_tophits"): ["-exclude", "genus", "-tophits"],
        ("tie", 2, "species"): ["-exclude", "species"],
        ("noanc", 2, "species"): ["-exclude", "species"]}
HOW = {"batch16": ["-batch", "16"], "host_reader": ["-reader", "host"]}
COL = "\t|\t"


def _norm(text):
    text = re.sub(r"^# time:    .*$", "# time:    T ms", text, flags=re.M)
    text = re.sub(r"^# speed:   .*$", "# speed:   S queries/min", text, flags=re.M)
    return sorted(text.split("\n"))


def _headers(tag):
    with open(os.path.join(GOLDEN, tag, "eval_headers.json")) as f:
        return json.load(f)


def _reads(fx, headers, d):
    for fn, seqs in (("r1.fq", fx.r1), ("r2.fq", fx.r2)):
        with open(d / fn, "w") as f:
            for n, s in zip(headers, seqs):
                f.write("@%s\n%s\n+\n%s\n" % (n, s, "I" * len(s)))


def _cli(pkg, fx, P, extra, cwd):
    prefix = fx.shard_paths[0][: -len(".db_0")]
    return subprocess.run([pkg.cli_path(), prefix, str(P), "r1.fq", "r2.fq", "-pairfiles", "-lowest", fx.q["lowest"], "-threads", "2",
                           "-maxcand", str(fx.maxcand), "-hitmin", "4", "-hitdiff", "80", "-out", "out.txt"] + extra,
                          cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)


@pytest.mark.parametrize("how", sorted(HOW))
@pytest.mark.parametrize("tag,P,name", sorted(RUNS))
def test_cli_exclusion_equals_the_references(tag, P, name, how, tmp_path):
    pkg = importlib.import_module("metacache-mpi_amd")
    pkg.build_host()
    fx = Fixture(tag, P)
    _reads(fx, _headers(tag), tmp_path)
    r = _cli(pkg, fx, P, RUNS[(tag, P, name)] + HOW[how], tmp_path)
    assert r.returncode == 0, r.stderr
    with gzip.open(os.path.join(os.path.dirname(fx.shard_paths[0]), "cli_excl_%s.out.gz" % name), "rt") as f:
        golden = f.read()
    assert _norm(open(tmp_path / "out.txt").read()) == _norm(golden)


class _Taxa:
    """nodes.dmp / names.dmp of a fixture: ranks, ranked lineages, scientific names"""

    def __init__(self, tag, host):
        d = os.path.join(GOLDEN, tag)
        self.parent, self.rank, self.name = {}, {}, {}
        for l in open(os.path.join(d, "nodes.dmp")):
            f = [x.strip() for x in l.split("|")]
            self.parent[int(f[0])] = int(f[1])
            self.rank[int(f[0])] = ROOT if int(f[0]) == 1 else host.rank_from_name(f[2])
        for l in open(os.path.join(d, "names.dmp")):
            f = [x.strip() for x in l.split("|")]
            if f[3] == "scientific name":
                self.name[int(f[0])] = f[1]
        self.by_text = {"%s:%s" % (host.lib().mcq_rank_name(self.rank[i]).decode(), self.name[i]): i for i in self.parent if self.rank[i] != RNONE}

    def lineage(self, i):
        lin = {}
        while True:
            if self.rank[i] != RNONE:
                lin.setdefault(self.rank[i], i)
            if self.parent[i] == i:
                return lin
            i = self.parent[i]

    def truth(self, header):
        """the taxon behind "taxid|", through its next ranked ancestor; None without one (src/classification.cpp:111-131)"""
        m = re.search(r"taxid\|(\d+)", header)
        i = int(m.group(1)) if m else 0
        if i not in self.parent:
            return None
        while self.rank[i] == RNONE and self.parent[i] != i:
            i = self.parent[i]
        return i if self.rank[i] != RNONE else None

    def lca_rank(self, a, b):
        if a is None or b is None:
            return RNONE
        la, lb = self.lineage(a), self.lineage(b)
        return next((r for r in range(ROOT + 1) if r in la and la[r] == lb.get(r)), RNONE)


@pytest.mark.parametrize("extra", [[], ["-exclude", "species"]], ids=["plain", "exclude_species"])
def test_cli_truth_column_and_precision(extra, tmp_path):
    pkg = importlib.import_module("metacache-mpi_amd")
    host = importlib.import_module("metacache-mpi_amd.host")
    pkg.build_host()
    fx = Fixture("mini", 4)
    headers = _headers("mini")
    _reads(fx, headers, tmp_path)
    r = _cli(pkg, fx, 4, ["-precision", "-ground-truth", "-batch", "64"] + extra, tmp_path)
    assert r.returncode == 0, r.stderr
    lines = open(tmp_path / "out.txt").read().split("\n")
    layout = [l for l in lines if l.startswith("# TABLE_LAYOUT: ")]
    assert layout == ["# TABLE_LAYOUT: query_header" + COL + "truth_rank:truth_taxname" + COL + "rank:taxname"]
    taxa = _Taxa("mini", host)
    truth = {h.split(" ")[0]: taxa.truth(h) for h in headers}
    assert sum(t is not None for t in truth.values()) > 100 and sum(t is None for t in truth.values()) > 1
    rows = [l.split(COL) for l in lines if l and not l.startswith("#")]
    assert len(rows) == len(headers) and all(len(c) == 3 for c in rows)
    triples = []
    text_of = {i: t for t, i in taxa.by_text.items()}
    for name, tcol, ccol in rows:
        t = truth[name]
        assert tcol == ("--" if t is None else text_of[t]), (name, tcol)
        best = None if ccol == "--" else taxa.by_text[ccol]
        triples.append((RNONE if best is None else taxa.rank[best], RNONE if t is None else taxa.rank[t], taxa.lca_rank(best, t)))
    start = next(i for i, l in enumerate(lines) if l.startswith("# unclassified: ") or l == "# classified:")
    assert "\n".join(lines[start:]) == _summary(*_restated(triples), "# ")
    assert "# ground truth known:" in lines and "# sensitivity (correctly classified / all) if ground truth known:" in lines
    if extra:                                                        # without its truth column, the reference's -exclude species run
        with gzip.open(os.path.join(os.path.dirname(fx.shard_paths[0]), "cli_excl_species.out.gz"), "rt") as f:
            ref = sorted(l for l in f.read().split("\n") if l and not l.startswith("#"))
        assert sorted(COL.join((c[0], c[2])) for c in rows) == ref


def test_cli_rejects_taxon_coverage(tmp_path):
    pkg = importlib.import_module("metacache-mpi_amd")
    pkg.build_host()
    fx = Fixture("mini", 4)
    _reads(fx, _headers("mini"), tmp_path)
    r = _cli(pkg, fx, 4, ["-taxon-coverage"], tmp_path)
    assert r.returncode != 0
    assert "-taxon-coverage is not supported" in r.stderr
    assert not os.path.exists(tmp_path / "out.txt")
    h = subprocess.run([pkg.cli_path(), "-help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert h.returncode != 0
    for word in ("-exclude RANK", "-ground-truth", "-precision", "-taxon-coverage", "mcq_query_mpi rejects"):
        assert word in h.stdout


def test_mpi_program_rejects_exclusion(tmp_path):
    """mcq_query_mpi shares the parser: it names mcq_query_cli and leaves before it opens a GPU or the database"""
    pkg = importlib.import_module("metacache-mpi_amd")
    pkg.build_host()
    mpiexec = shutil.which("mpiexec") or "/opt/conda/bin/mpiexec"
    if not os.path.exists(pkg.mpi_cli_path()) or not os.path.exists(mpiexec):
        pytest.skip("no MPI on this box")
    env = dict(os.environ, LD_LIBRARY_PATH=pkg.mpi_lib_dir() + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    for opt in (["-exclude", "species"], ["-ground-truth"], ["-precision"]):
        r = subprocess.run([mpiexec, "-n", "1", pkg.mpi_cli_path(), str(tmp_path / "no_such_db"), "4", "r1.fq", "r2.fq"] + opt,
                           cwd=tmp_path, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
        assert r.returncode != 0, opt
        assert "options of mcq_query_cli" in r.stderr and "no_such_db" not in r.stderr, (opt, r.stderr)
