"""mcq_query_cli -align on the mini fixture's P = 4 shard files with the options of the reference run that made
tests/golden/mini/P4/cli_align.out.gz and cli_seq_plain.out.gz (tests/golden/make_golden_alignment.py): the -out file equals the
reference's after sorting by whole records -- a mapping line with its three block lines is one record --, the two timing lines
left out.  Then the options around it: -mapped-only, -nomap, a rank above sequence, a genome file that is not there, and
-align-candidate-range, whose ranges must be those mcq_target_hits gives for the top target."""
import gzip
import importlib
import os
import re
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (first: the library then binds to the HIP runtime torch brings along)

import align_ref
from golden_util import Fixture
from oracle import dbfile
from oracle import mc_oracle as orc
from test_align_ref import GOLDEN, load_genomes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_OPTS = ["-lowest", "sequence", "-threads", "2", "-maxcand", "4", "-hitmin", "4", "-hitdiff", "80"]
PARAM_LINE = "# Query sequences will be aligned to best candidate target => SLOW!"
STRIDE, WINLEN = 113, 128       # target windows of the mini fixture


def _pkg():
    return importlib.import_module("metacache-mpi_amd")


def records(text):
    """the lines of an -out file as records, the two timing lines left out, sorted"""
    lines = [l for l in text.split("\n") if not l.startswith("# time:    ") and not l.startswith("# speed:   ")]
    out, i = [], 0
    while i < len(lines):
        n = 4 if (not lines[i].startswith("#") and i + 3 < len(lines) and lines[i + 1].startswith("#   score  ")) else 1
        out.append("\n".join(lines[i:i + n]))
        i += n
    return sorted(out)


def blocks(text):
    """{read header: (mapping line, score, file, index, range begin, range end, aligned query, aligned target)}"""
    lines = text.split("\n")
    out = {}
    for i, l in enumerate(lines):
        m = re.match(r"#   score  (-?\d+)  aligned to (.*) #(\d+) in range \[(\d+),(\d+)\]$", l)
        if m:
            out[lines[i - 1].split("\t|\t")[0]] = (lines[i - 1], int(m.group(1)), m.group(2), int(m.group(3)), int(m.group(4)), int(m.group(5)),
                                                    lines[i + 1][len("#   query  "):], lines[i + 2][len("#   target "):])
    return out


def mapping(text):
    return {l.split("\t|\t")[0]: l for l in text.split("\n") if l and not l.startswith("#")}


def golden(name):
    with gzip.open(os.path.join(GOLDEN, "mini", "P4", name), "rt") as f:
        return f.read()


_runs = {}


def run_cli(tmp_path_factory, extra=(), genomes=True, opts=REF_OPTS):
    """(return code, -out text, stderr) of one run in a working directory of its own; a run is made once per module"""
    key = (tuple(extra), genomes, tuple(opts))
    if key not in _runs:
        pkg = _pkg()
        fx = Fixture("mini", 4)
        cwd = tmp_path_factory.mktemp("cli_align")
        for fn, seqs in (("r1.fq", fx.r1), ("r2.fq", fx.r2)):
            with open(cwd / fn, "w") as f:
                for n, s in zip(fx.names, seqs):
                    f.write("@%s\n%s\n+\n%s\n" % (n, s, "I" * len(s)))
        if genomes:                                     # the name the shard files store, relative to the working directory
            os.makedirs(cwd / "genomes")
            with gzip.open(os.path.join(GOLDEN, "mini", "genomes.fa.gz"), "rt") as f, open(cwd / "genomes" / "all.fna", "w") as o:
                o.write(f.read())
        prefix = fx.shard_paths[0][: -len(".db_0")]
        r = subprocess.run([pkg.cli_path(), prefix, "4", "r1.fq", "r2.fq"] + list(opts) + ["-out", "out.txt"] + list(extra),
                           cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
        _runs[key] = (r.returncode, open(cwd / "out.txt").read() if os.path.exists(cwd / "out.txt") else "", r.stderr)
    return _runs[key]


@pytest.mark.gpu
def test_align_out_file_equals_the_references(tmp_path_factory):
    rc, plain, err = run_cli(tmp_path_factory)
    assert rc == 0, err
    rc, mine, err = run_cli(tmp_path_factory, ["-align"])
    assert rc == 0, err
    ref_plain, ref = golden("cli_seq_plain.out.gz"), golden("cli_align.out.gz")
    assert PARAM_LINE in mine.split("\n")
    if records(plain) == records(ref_plain):
        assert records(mine) == records(ref)
        return
    # the plain run differs already: a finding about -lowest sequence, not about -align.  The blocks of the reads whose mapping
    # lines agree must be the reference's, and those reads must carry at least nine tenths of its 132 blocks
    mp, rp = mapping(plain), mapping(ref_plain)
    agree = {h for h in rp if mp.get(h) == rp[h]}
    mb, rb = blocks(mine), blocks(ref)
    assert len(rb) == 132
    want = {h: b for h, b in rb.items() if h in agree}
    print("mapping lines that agree with the reference's plain run: %d of %d; reference blocks among them: %d of %d"
          % (len(agree), len(rp), len(want), len(rb)))
    assert 10 * len(want) >= 9 * len(rb)
    for h, b in want.items():
        assert mb.get(h) == b, h


@pytest.mark.gpu
def test_mapped_only_and_nomap(tmp_path_factory):
    rc, full, err = run_cli(tmp_path_factory, ["-align"])
    assert rc == 0, err
    rc, mo, err = run_cli(tmp_path_factory, ["-align", "-mapped-only"])
    assert rc == 0, err
    keep = [r for r in records(full) if r.startswith("#") or not r.split("\n")[0].endswith("\t|\t--")]
    assert records(mo) == keep and len(blocks(mo)) == len(blocks(full)) > 0
    rc, nm, err = run_cli(tmp_path_factory, ["-align", "-nomap"])
    assert rc == 0, err
    assert PARAM_LINE in nm.split("\n") and not mapping(nm) and "#   score  " not in nm


@pytest.mark.gpu
def test_above_sequence_level_only_the_parameter_line(tmp_path_factory):
    opts = ["-lowest", "species"] + REF_OPTS[2:]
    rc, plain, err = run_cli(tmp_path_factory, opts=opts)
    assert rc == 0, err
    rc, mine, err = run_cli(tmp_path_factory, ["-align"], genomes=False, opts=opts)       # (no genome file is asked for either)
    assert rc == 0 and "-align" not in err, err
    assert "#   score  " not in mine
    assert records(mine) == sorted(records(plain) + [PARAM_LINE])


@pytest.mark.gpu
def test_a_missing_genome_file_gives_no_block_and_one_stderr_line(tmp_path_factory):
    rc, plain, err = run_cli(tmp_path_factory)
    assert rc == 0, err
    rc, mine, err = run_cli(tmp_path_factory, ["-align"], genomes=False)
    assert rc == 0, err
    assert [l for l in err.split("\n") if l].count("-align: can't open file genomes/all.fna: its sequences get no alignment") == 1
    assert "#   score  " not in mine
    assert records(mine) == sorted(records(plain) + [PARAM_LINE])


@pytest.mark.gpu
def test_align_candidate_range(tmp_path_factory):
    eng = importlib.import_module("metacache-mpi_amd.engine")
    rc, zero, err = run_cli(tmp_path_factory, ["-align"])
    assert rc == 0, err
    rc, mine, err = run_cli(tmp_path_factory, ["-align", "-align-candidate-range"])
    assert rc == 0, err
    zb, mb = blocks(zero), blocks(mine)
    assert set(zb) == set(mb) and len(mb) > 0
    assert mapping(zero) == mapping(mine)                       # the option is written into nothing but the blocks
    assert [l for l in zero.split("\n") if l.startswith("#") and not l.startswith("#   ") and not l.startswith("# time") and not l.startswith("# speed")] == \
           [l for l in mine.split("\n") if l.startswith("#") and not l.startswith("#   ") and not l.startswith("# time") and not l.startswith("# speed")]
    # the top target's range from mcq_target_hits, one slot per read
    fx = Fixture("mini", 4)
    keys, off, locs = dbfile.union_shards(fx.shards)
    p = fx.params
    db = eng.Database(keys, off, locs, fx.tax.target_keys(fx.n_targets, 0), k=p["qk"], sketch_size=p["qs"], winlen=p["qwinlen"],
                      winstride=p["qwinstride"], tgt_winstride=p["winstride"])
    ws = eng.Workspace(db, len(fx.names), sum(len(s) for s in fx.interleaved()) + 64)
    rb, ro = orc.pack_reads(fx.interleaved())
    order = [h for h in fx.names if h in mb]
    targets = np.full((len(fx.names), 1), eng.MCQ_TARGET_UNUSED, np.uint32)
    for h in order:
        targets[fx.names.index(h), 0] = mb[h][3] - 1          # record index in the one genome file = target + 1
    rng, cnt, st = ws.target_hits_host(rb, ro, True, targets)
    genomes = load_genomes()
    assert (p["winstride"], p["winlen"]) == (STRIDE, WINLEN)
    differ = 0
    for h in order:
        q = fx.names.index(h)
        line, score, fname, index, rbeg, rend, aq, at = mb[h]
        tgt, hits, beg, n_win = rng[q, 0].tolist()
        assert n_win > 0 and (rbeg, rend) == (STRIDE * beg, STRIDE * (beg + n_win - 1) + STRIDE), (h, rng[q, 0], rbeg, rend)
        g = genomes[index - 1]
        subject = g[STRIDE * beg: min(len(g), STRIDE * (beg + n_win - 1) + WINLEN)]
        e = align_ref.make_semi_global_alignment(fx.r1[q].encode(), fx.r2[q].encode(), subject)
        assert (score, aq.encode(), at.encode()) == e[:3], h
        differ += mb[h][1:] != zb[h][1:]
    assert differ > 0


def test_mcq_query_mpi_rejects_align():
    """without a GPU: the option is refused before any GPU work, with a line that names mcq_query_cli"""
    import shutil
    pkg = _pkg()
    pkg.build_host()
    mpiexec = shutil.which("mpiexec") or "/opt/conda/bin/mpiexec"
    build = importlib.import_module("metacache-mpi_amd.build")
    if not os.path.exists(mpiexec) or not os.path.exists(os.path.join(build._MPI_ROOT, "include", "mpi.h")) or \
            not os.path.exists(os.path.join(build._MPI_ROOT, "lib", build._MPI_LIBS[0])):
        pytest.skip("no MPI on this box")
    assert os.path.exists(pkg.mpi_cli_path()), "an MPI is installed, but build_host() left no mcq_query_mpi"
    env = dict(os.environ, LD_LIBRARY_PATH=pkg.mpi_lib_dir() + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    for name in ("-align", "-alignment", "-showalignment"):
        r = subprocess.run([mpiexec, "-n", "1", pkg.mpi_cli_path(), "nodb", "4", "r1.fq", "r2.fq", "-lowest", "sequence", name],
                           env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
        assert r.returncode == 2, (r.returncode, r.stderr)
        assert "-align is an option of mcq_query_cli" in r.stderr
