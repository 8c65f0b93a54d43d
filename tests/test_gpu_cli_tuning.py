"""The database query options through the CLIs: -winlen, -winstride, -sketchlen, -max-locations-per-feature,
-remove-overpopulated-features (get_database_query_options, src/query_options.cpp:41-66; src/mode_query.cpp:354-387).

mcq_query_cli writes, for every run of tests/golden/make_golden_tuning.py, the -out file the reference wrote under
mpiexec -n P (tests/golden/<set>/P<n>/cli_tune_*.out.gz): compared as tests/test_gpu_cli.py compares -- lines sorted,
everything byte for byte except the measured values of "# time:" and "# speed:".  Every fixture but maxlocs1 differs from
the untuned run of the reference in at least one mapping line (the generator stops otherwise), so a program that skips the
options fails here."""
import gzip
import importlib
import os
import re
import shutil
import subprocess

import pytest

from golden_util import Fixture

pytestmark = pytest.mark.gpu

MAXLOCS = ["-max-locations-per-feature"]
REMOVE = ["-remove-overpopulated-features"]
# (set, P, name, -lowest, options): the table of tests/golden/make_golden_tuning.py
RUNS = [("overpop", 2, "maxlocs40", "sequence", MAXLOCS + ["40"]),
        ("overpop", 4, "remove40", "species", REMOVE + MAXLOCS + ["40"]),
        ("overpop", 2, "remove1", "sequence", REMOVE + MAXLOCS + ["1"]),
        ("overpop", 2, "maxlocs1", "sequence", MAXLOCS + ["1"]),
        ("mini", 2, "maxlocs2", "sequence", MAXLOCS + ["2"]),
        ("mini", 4, "win64_sketch8", "sequence", ["-winlen", "64", "-sketchlen", "8"]),
        ("mini", 2, "win100_stride50", "sequence", ["-winlen", "100", "-winstride", "50"]),
        ("mini", 4, "stride32", "sequence", ["-winstride", "32"])]


def _pkg():
    pkg = importlib.import_module("metacache-mpi_amd")
    pkg.build_host()
    return pkg


def norm(text):
    text = re.sub(r"^# time:    .*$", "# time:    T ms", text, flags=re.M)
    text = re.sub(r"^# speed:   .*$", "# speed:   S queries/min", text, flags=re.M)
    return sorted(text.split("\n"))


def golden(fx, name):
    with gzip.open(os.path.join(os.path.dirname(fx.shard_paths[0]), name), "rt") as f:
        return f.read()


def write_reads(fx, cwd):
    for fn, seqs in (("r1.fq", fx.r1), ("r2.fq", fx.r2)):
        with open(cwd / fn, "w") as f:
            for n, s in zip(fx.names, seqs):
                f.write("@%s\n%s\n+\n%s\n" % (n, s, "I" * len(s)))


def base_opts(fx, lowest):
    return ["-lowest", lowest, "-tophits", "-threads", "2", "-maxcand", str(fx.maxcand), "-hitmin", "4", "-hitdiff", "80"]


def run_cli(fx, P, cwd, opts, env=None):
    return subprocess.run([_pkg().cli_path(), fx.shard_paths[0][: -len(".db_0")], str(P), "r1.fq", "r2.fq"] + opts + ["-out", "out.txt"],
                          cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)


@pytest.mark.parametrize("tag,P,name,lowest,extra", RUNS, ids=[r[2] for r in RUNS])
def test_cli_writes_the_references_tuned_out_file(tag, P, name, lowest, extra, tmp_path):
    fx = Fixture(tag, P)
    write_reads(fx, tmp_path)
    r = run_cli(fx, P, tmp_path, base_opts(fx, lowest) + extra)
    assert r.returncode == 0, r.stderr
    assert norm(open(tmp_path / "out.txt").read()) == norm(golden(fx, "cli_tune_%s.out.gz" % name))
    if "-max-locations-per-feature" in extra and name != "maxlocs1":
        assert re.search(r"bucket rule: \d+ buckets shrunk, \d+ removed", r.stderr), r.stderr


def test_mpi_program_takes_the_options_through_the_same_lines(tmp_path):
    """two ranks on one GPU (-transport mpi): every rank streams all shard files, applies the rule per chunk and keeps its
    hash range; the window options reach both descriptors"""
    pkg = _pkg()
    mpiexec = shutil.which("mpiexec") or "/opt/conda/bin/mpiexec"
    if not os.path.exists(pkg.mpi_cli_path()) or not os.path.exists(mpiexec):
        pytest.skip("no MPI on this box")
    env = dict(os.environ, LD_LIBRARY_PATH=pkg.mpi_lib_dir() + ":" + os.environ.get("LD_LIBRARY_PATH", ""), HSA_ENABLE_IPC_MODE_LEGACY="0")
    for tag, P, name, lowest, extra in (RUNS[1], RUNS[5]):
        fx = Fixture(tag, P)
        cwd = tmp_path / name
        cwd.mkdir()
        write_reads(fx, cwd)
        r = subprocess.run([mpiexec, "-n", "2", pkg.mpi_cli_path(), fx.shard_paths[0][: -len(".db_0")], str(P), "r1.fq", "r2.fq"] +
                           base_opts(fx, lowest) + extra + ["-transport", "mpi", "-out", "out.txt"],
                           cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
        assert norm(open(cwd / "out.txt").read()) == norm(golden(fx, "cli_tune_%s.out.gz" % name))


@pytest.mark.parametrize("extra,word", [(["-winlen", "200"], "128"), (["-winlen", "8"], "k = 16"), (["-sketchlen", "64"], "32")])
def test_values_outside_the_engines_limits_abort_before_anything_is_written(extra, word, tmp_path):
    fx = Fixture("mini", 4)
    write_reads(fx, tmp_path)
    r = run_cli(fx, 4, tmp_path, base_opts(fx, "sequence") + extra)
    assert r.returncode != 0
    abort = [l for l in r.stderr.split("\n") if l.startswith("ABORT:")]
    assert abort and word in abort[0] and extra[0] in abort[0], r.stderr
    assert not os.path.exists(tmp_path / "out.txt")


def test_without_the_options_nothing_changes_on_either_route(tmp_path):
    """a guard: the existing -tophits fixture, by the host-side union and by the streaming route"""
    fx = Fixture("mini", 4)
    write_reads(fx, tmp_path)
    opts = ["-lowest", fx.q["lowest"], "-maxcand", str(fx.maxcand), "-hitmin", str(fx.hitmin), "-hitdiff", str(fx.q["hitdiff"]), "-threads", "2", "-tophits"]
    for env in (None, dict(os.environ, MCQ_STREAM_LOAD_MIN_MB="0")):
        r = run_cli(fx, 4, tmp_path, opts, env)
        assert r.returncode == 0, r.stderr
        assert "bucket rule" not in r.stderr
        assert norm(open(tmp_path / "out.txt").read()) == norm(golden(fx, "cli_tophits.out.gz"))
        os.remove(tmp_path / "out.txt")


def test_help_names_the_five_options():
    h = subprocess.run([_pkg().cli_path(), "-help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    for word in ("-winlen", "-winstride", "-sketchlen", "-max-locations-per-feature", "-remove-overpopulated-features", "-max-load-fac", "128", "32"):
        assert word in h.stdout, word
