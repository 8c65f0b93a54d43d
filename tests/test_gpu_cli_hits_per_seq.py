"""mcq_query_cli -hits-per-seq [FILE]: the per-reference window hit lists (show_matches_per_targets, src/printing.cpp:437-469)
and the query_id column.  The reference's MPI program prints the header lines only (its call that fills the table is commented
out), so the expected table is the Python restatement (tests/hits_table_ref.py) fed from the oracle's candidates and matches."""
import gzip
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import hits_table_ref as ref
from golden_util import Fixture
from oracle import dbfile
from oracle import mc_oracle as orc

pytestmark = pytest.mark.gpu
COL = "\t|\t"
HEAD3 = ["# --- list of hits for each reference sequence ---",
         "# window start position within sequence = window_index * window_stride(=%d)",
         "# TABLE_LAYOUT:  sequence " + COL + " windows_in_sequence " + COL + "queryid/window_index:hits/window_index:hits/...,queryid/..."]


def _pkg():
    pkg = importlib.import_module("metacache-mpi_amd")
    pkg.build_host()
    return pkg


def _write_reads(fx, d):
    for fn, seqs in (("r1.fq", fx.r1), ("r2.fq", fx.r2)):
        with open(d / fn, "w") as f:
            for n, s in zip(fx.names, seqs):
                f.write("@%s\n%s\n+\n%s\n" % (n, s, "I" * len(s)))


def _run(pkg, fx, d, extra, lowest="sequence"):
    prefix = fx.shard_paths[0][: -len(".db_0")]
    r = subprocess.run([pkg.cli_path(), prefix, str(fx.P), "r1.fq", "r2.fq", "-lowest", lowest, "-maxcand", str(fx.maxcand),
                        "-hitmin", str(fx.hitmin), "-hitdiff", str(fx.q["hitdiff"]), "-threads", "2", "-out", "out.txt"] + extra,
                       cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r, open(d / "out.txt").read()


_expected = {}


def expected_table(fx, quirks):
    """the table of the restatement from the oracle's candidates (as the run folds them: P ranks, the u32 wire format's quirk)
    and matches; computed once per fixture"""
    key = (fx.tag, fx.P, quirks)
    if key not in _expected:
        keys, off, locs = dbfile.union_shards(fx.shards)
        p = fx.params
        t2t = fx.tax.target_keys(fx.n_targets, 0)
        tgt_of = {int(k): t for t, k in enumerate(t2t)}
        odb = orc.OracleDb(keys, off, locs, t2t, k=p["qk"], s=p["qs"], winlen=p["qwinlen"], winstride=p["qwinstride"], tgt_winstride=p["winstride"])
        bases, seq_off = orc.pack_reads(fx.interleaved())
        cand, ncand = odb.query(bases, seq_off, True, max_cand=fx.maxcand, emulate_ranks=fx.P, quirk_seq_drop=1 if quirks else 0)
        tab = ref.RefHitsTable()
        for q, (a, b) in enumerate(zip(fx.r1, fx.r2)):
            per_target = {int(t): (int(h), int(bg), int(en)) for t, h, bg, en in odb.target_cands(a, b, 0)}
            cs = []
            for tax, hits, _, _ in cand[q, :ncand[q]].tolist():
                assert tax & 0x80000000                   # -lowest sequence: every candidate is a target
                t = tgt_of[tax]
                assert per_target[t][0] == hits
                cs.append((t, hits, per_target[t][1], per_target[t][2]))
            tab.insert(q + 1, odb.matches(a, b), cs, fx.hitmin)
        assert tab.per_target                             # the case has rows
        _expected[key] = ref.table_text(tab, fx.tax, ref.windows_of_targets(fx), p["qwinstride"])
    return _expected[key]


def _split(text):
    """(lines in front of the table, the table's lines, lines behind it)"""
    lines = text.split("\n")
    i = lines.index(HEAD3[0])
    j = i + 3
    while j < len(lines) and lines[j] and not lines[j].startswith("#"):
        j += 1
    return lines[:i], lines[i:j], lines[j:]


def _check_head_and_ids(fx, front):
    assert "# A list of hits per reference sequence will be generated after the read mapping." in front
    assert "# A list of absolute and relative abundances per taxon will be generated after the read mapping." in front
    layout = [l for l in front if l.startswith("# TABLE_LAYOUT: ")]
    assert layout == ["# TABLE_LAYOUT: query_id" + COL + "query_header" + COL + "rank:taxname"]
    maps = [l for l in front if l and not l.startswith("#")]
    assert len(maps) == len(fx.names)
    for i, l in enumerate(maps):                          # every mapping line carries its 1-based id
        assert l.split(COL)[:2] == [str(i + 1), fx.names[i]], l
    return maps


@pytest.mark.parametrize("tag,quirks", [("mini", True), ("tie", True), ("mini", False)])
def test_table_equals_the_restatement(tag, quirks, tmp_path):
    pkg = _pkg()
    fx = Fixture(tag, 2)
    _write_reads(fx, tmp_path)
    want = expected_table(fx, quirks).split("\n")
    assert want[:3] == [HEAD3[0], HEAD3[1] % fx.params["qwinstride"], HEAD3[2]]
    q = [] if quirks else ["-noquirks"]
    r, text = _run(pkg, fx, tmp_path, ["-hits-per-seq"] + q)
    front, table, back = _split(text)
    maps = _check_head_and_ids(fx, front)
    assert table[:3] == want[:3] and sorted(table) == sorted(l for l in want if l)
    assert table[3:] == [l for l in want[3:] if l]            # (and in this project's own row order: ascending target)
    assert any(l.startswith("# queries: ") for l in back)    # the summary follows the table

    # -hits-per-seq FILE: the table goes to FILE, the rest stays as it was; -batch 16 and -reader host change nothing
    for extra in (["-hits-per-seq", "hits.txt"], ["-hits-per-seq", "hits.txt", "-batch", "16"], ["-hits-per-seq", "hits.txt", "-reader", "host"],
                  ["-hits-per-seq", "out.txt"]):                     # FILE = the -out file: cleared, the table stays in the -out file
        if os.path.exists(tmp_path / "hits.txt"):
            os.remove(tmp_path / "hits.txt")
        r2, text2 = _run(pkg, fx, tmp_path, extra + q)
        mask = lambda t: re.sub(r"^# (time:    |speed:   ).*$", "# T", t, flags=re.M)
        if extra[1] == "out.txt":
            assert mask(text2) == mask(text) and not os.path.exists(tmp_path / "hits.txt")
            continue
        assert "Per-Target mappings will be written to file: hits.txt" in r2.stdout
        assert open(tmp_path / "hits.txt").read().split("\n") == table + [""], extra
        assert HEAD3[0] not in text2
        assert mask(text2).split("\n") == mask("\n".join(front + back)).split("\n"), extra


def test_sequence_column_is_what_the_mapping_lines_print(tmp_path):
    """the table's show_taxon lives in the host library, the mapping lines' in the CLI (Out::best): with the lineage on and ids
    shown, the sequence column of a row must be, character for character, the classification column of the reads that were
    classified as that sequence"""
    pkg = _pkg()
    fx = Fixture("mini", 2)
    _write_reads(fx, tmp_path)
    for extra in (["-lineage", "-taxids"], ["-lineage", "-taxids", "-highest", "family"], ["-lineage", "-omit-ranks"], ["-taxids-only"]):
        r, text = _run(pkg, fx, tmp_path, ["-hits-per-seq"] + extra)
        front, table, back = _split(text)
        cls = {l.split(COL)[-1] for l in front if l and not l.startswith("#")}
        first = lambda col: col.split(",")[0]
        by_first = {}
        for c in cls:
            by_first.setdefault(first(c), set()).add(c)
        rows = [l.split(COL)[0] for l in table[3:]]
        met = [row for row in rows if first(row) in by_first]
        assert len(met) >= 1, (extra, rows[:3], sorted(cls)[:3])             # some sequence is a read's classification: the comparison is not empty
        for row in met:
            assert by_first[first(row)] == {row}, (extra, row, by_first[first(row)])


@pytest.mark.parametrize("tag,P", [("mini", 4), ("tie", 2)])
def test_lowest_above_sequence_gives_headers_only(tag, P, tmp_path):
    """candidates above sequence level are skipped (src/matches_per_target.h:117-123): with -lowest species the table is its three
    header lines, and the mapping lines without their id column are the reference's own"""
    pkg = _pkg()
    fx = Fixture(tag, P)
    _write_reads(fx, tmp_path)
    r, text = _run(pkg, fx, tmp_path, ["-hits-per-seq"], lowest=fx.q["lowest"])
    front, table, back = _split(text)
    assert table == [HEAD3[0], HEAD3[1] % fx.params["qwinstride"], HEAD3[2]]
    maps = [l for l in front if l and not l.startswith("#")]
    assert [l.split(COL)[0] for l in maps] == [str(i + 1) for i in range(len(fx.names))]
    with gzip.open(os.path.join(os.path.dirname(fx.shard_paths[0]), "cli_default.out.gz"), "rt") as f:
        ref_maps = [l for l in f.read().split("\n") if l and not l.startswith("#")]
    assert sorted(l.split(COL, 1)[1] for l in maps) == sorted(ref_maps)


def test_mpi_program_rejects_the_option(tmp_path):
    pkg = _pkg()
    mpiexec = shutil.which("mpiexec") or "/opt/conda/bin/mpiexec"
    if not os.path.exists(pkg.mpi_cli_path()) or not os.path.exists(mpiexec):
        pytest.skip("no MPI on this box")
    fx = Fixture("mini", 2)
    _write_reads(fx, tmp_path)
    env = dict(os.environ, LD_LIBRARY_PATH=pkg.mpi_lib_dir() + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([mpiexec, "-n", "1", pkg.mpi_cli_path(), fx.shard_paths[0][: -len(".db_0")], "2", "r1.fq", "r2.fq", "-hits-per-seq"],
                       cwd=tmp_path, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode != 0
    assert "-hits-per-seq" in r.stderr and "mcq_query_cli" in r.stderr and r.stderr.count("\n") == 1
