"""-abundances / -abundance-per through mcq_query_cli and mcq_query_mpi: the whole -out file (and the -abundances FILE)
against what the reference wrote for the same options (tests/golden/*/P*/cli_abund_*, make_golden_abundance.py)."""
import gzip
import importlib
import os
import re
import shutil
import subprocess

import pytest

from golden_util import Fixture

pytestmark = pytest.mark.gpu

VARIANTS = {
    "species": ["-abundance-per", "species"],                     # the reference's scripted command line
    "both_genus": ["-abundances", "-abundance-per", "genus"],
    "seq": ["-abundance-per", "sequence"],
    "file": ["-abundances", "ab.txt", "-abundance-per", "species"],
    "nomap": ["-nomap", "-abundance-per", "species"],
}


def _norm(text):
    text = re.sub(r"^# time:    .*$", "# time:    T ms", text, flags=re.M)
    text = re.sub(r"^# speed:   .*$", "# speed:   S queries/min", text, flags=re.M)
    return sorted(text.split("\n"))


def _golden(fx, name):
    with gzip.open(os.path.join(os.path.dirname(fx.shard_paths[0]), name), "rt") as f:
        return f.read()


def _reads(fx, d):
    for fn, seqs in (("r1.fq", fx.r1), ("r2.fq", fx.r2)):
        with open(d / fn, "w") as f:
            for n, s in zip(fx.names, seqs):
                f.write("@%s\n%s\n+\n%s\n" % (n, s, "I" * len(s)))


@pytest.mark.parametrize("tag,P", [("mini", 4), ("tie", 2)])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_cli_abundances_equal_the_references(tag, P, variant, tmp_path):
    pkg = importlib.import_module("metacache-mpi_amd")
    pkg.build_host()
    fx = Fixture(tag, P)
    _reads(fx, tmp_path)
    prefix = fx.shard_paths[0][: -len(".db_0")]
    r = subprocess.run([pkg.cli_path(), prefix, str(P), "r1.fq", "r2.fq", "-pairfiles", "-lowest", fx.q["lowest"], "-threads", "2",
                        "-maxcand", str(fx.maxcand), "-hitmin", "4", "-hitdiff", "80", "-out", "out.txt"] + VARIANTS[variant],
                       cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert _norm(open(tmp_path / "out.txt").read()) == _norm(_golden(fx, "cli_abund_%s.out.gz" % variant))
    if variant == "file":
        assert open(tmp_path / "ab.txt").read() == _golden(fx, "cli_abund_file.ab.txt.gz")


def test_cli_abundances_to_stdout_and_batches(tmp_path):
    """without -out the tables go to stdout; cut into batches the counts stay the same"""
    pkg = importlib.import_module("metacache-mpi_amd")
    fx = Fixture("mini", 4)
    _reads(fx, tmp_path)
    prefix = fx.shard_paths[0][: -len(".db_0")]
    r = subprocess.run([pkg.cli_path(), prefix, "4", "r1.fq", "r2.fq", "-lowest", "species", "-maxcand", "4", "-hitmin", "4",
                        "-hitdiff", "80", "-threads", "2", "-batch", "16", "-abundances", "-abundance-per", "genus"],
                       cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert _norm(r.stdout) == _norm(_golden(fx, "cli_abund_both_genus.out.gz"))


def test_mpi_program_abundances(tmp_path):
    """mcq_query_mpi -n 2 -transport mpi: every rank classifies its slice on its GPU, the counts are reduced to rank 0"""
    pkg = importlib.import_module("metacache-mpi_amd")
    pkg.build_host()
    mpiexec = shutil.which("mpiexec") or "/opt/conda/bin/mpiexec"
    if not os.path.exists(pkg.mpi_cli_path()) or not os.path.exists(mpiexec):
        pytest.skip("no MPI on this box")
    fx = Fixture("mini", 4)
    _reads(fx, tmp_path)
    prefix = fx.shard_paths[0][: -len(".db_0")]
    env = dict(os.environ, LD_LIBRARY_PATH=pkg.mpi_lib_dir() + ":" + os.environ.get("LD_LIBRARY_PATH", ""), HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([mpiexec, "-n", "2", pkg.mpi_cli_path(), prefix, "4", "r1.fq", "r2.fq", "-lowest", fx.q["lowest"],
                        "-maxcand", str(fx.maxcand), "-hitmin", "4", "-hitdiff", "80", "-threads", "2", "-transport", "mpi",
                        "-abundance-per", "species", "-out", "out.txt"],
                       cwd=tmp_path, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    assert _norm(open(tmp_path / "out.txt").read()) == _norm(_golden(fx, "cli_abund_species.out.gz"))
