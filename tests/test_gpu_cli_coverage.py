"""mcq_query_cli -coverage [FILE] and -cov-percentile P.

(a) The report of a run must be what the -hits-per-seq table the SAME run printed adds up to: that table is pinned to the oracle by
tests/test_gpu_cli_hits_per_seq.py, and it is made from the very ranges and count rows the coverage accumulator folds.
(b) The cut is the restatement's (tests/coverage_ref.py) over part (a)'s numbers, and the second pass is a query against the database
without the removed sequences' locations: OracleDb.reduce_query on OracleDb.matches minus those targets, the construction of
tests/test_gpu_exclusion.py.  (c) Rejections and notices."""
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import coverage_ref as ref
from golden_util import Fixture
from oracle import dbfile
from oracle import mc_oracle as orc

pytestmark = pytest.mark.gpu
COL = "\t|\t"
HITS_HEAD = "# --- list of hits for each reference sequence ---"
COV_HEAD = "# " + ref.HEAD
FIXTURES = [("mini", 2), ("tie", 2)]
_state = {}


def _pkg():
    if "pkg" not in _state:
        pkg = importlib.import_module("metacache-mpi_amd")
        pkg.build_host()
        _state["pkg"] = pkg
    return _state["pkg"]


def _write_reads(fx, d):
    for fn, seqs in (("r1.fq", fx.r1), ("r2.fq", fx.r2)):
        with open(os.path.join(d, fn), "w") as f:
            for n, s in zip(fx.names, seqs):
                f.write("@%s\n%s\n+\n%s\n" % (n, s, "I" * len(s)))


def _cmd(pkg, fx, extra, lowest="sequence"):
    return [pkg.cli_path(), fx.shard_paths[0][: -len(".db_0")], str(fx.P), "r1.fq", "r2.fq", "-lowest", lowest, "-maxcand", str(fx.maxcand),
            "-hitmin", str(fx.hitmin), "-hitdiff", str(fx.q["hitdiff"]), "-threads", "2", "-out", "out.txt"] + extra


def _run(pkg, fx, d, extra, lowest="sequence"):
    r = subprocess.run(_cmd(pkg, fx, extra, lowest), cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    with open(os.path.join(d, "out.txt")) as f:
        return r, f.read()


def _block(lines, head):
    """the lines of the block that starts with `head`: its # lines, then its rows"""
    i = lines.index(head)
    j = i + 1
    while j < len(lines) and lines[j].startswith("#") and not lines[j].startswith("# ---"):
        j += 1
    while j < len(lines) and lines[j] and not lines[j].startswith("#"):
        j += 1
    return i, j


def _from_hits_table(rows):
    """{sequence column: (windows_in_sequence, distinct windows, entries, sum of hits)} of the -hits-per-seq table's rows"""
    out = {}
    for l in rows:
        seq, windows, entries = l.split(COL)
        wins, n, hits = set(), 0, 0
        for e in entries.split(","):
            n += 1
            for wh in e.split("/")[1:]:
                w, h = wh.split(":")
                wins.add(int(w)); hits += int(h)
        out[seq] = (int(windows), len(wins), n, hits)
    return out


def _world(tag, P, tmp_path_factory):
    """one fixture: its reads on disk, the run with -hits-per-seq -coverage cov.txt, and the names of its targets (made once)"""
    if (tag, P) not in _state:
        pkg = _pkg()
        host = importlib.import_module("metacache-mpi_amd.host")
        fx = Fixture(tag, P)
        d = str(tmp_path_factory.mktemp("cov_" + tag))
        _write_reads(fx, d)
        r, text = _run(pkg, fx, d, ["-hits-per-seq", "-coverage", "cov.txt"])
        rdb = host.RefDb(fx.shard_paths[0][: -len(".db_0")], P)
        seq_col = ["sequence:" + rdb.taxon_name(rdb.target_key(t)) for t in range(fx.n_targets)]
        assert len(set(seq_col)) == fx.n_targets
        with open(os.path.join(d, "cov.txt")) as f:
            report = f.read()
        _state[(tag, P)] = dict(pkg=pkg, fx=fx, d=d, stdout=r.stdout, text=text, report=report, seq_col=seq_col,
                                windows=rdb.seq_windows().tolist(), rdb=rdb)
    return _state[(tag, P)]


@pytest.mark.parametrize("tag,P", FIXTURES)
def test_report_is_what_the_hits_table_adds_up_to(tag, P, tmp_path_factory):
    w = _world(tag, P, tmp_path_factory)
    lines = w["text"].split("\n")
    assert "Per-sequence coverage will be written to file: cov.txt" in w["stdout"] and COV_HEAD not in lines
    assert "# A list of window coverage per reference sequence will be generated after the read mapping." in lines
    i, j = _block(lines, HITS_HEAD)
    table = _from_hits_table(lines[i + 3:j])
    assert len(table) >= 2
    rep = w["report"].split("\n")
    assert rep[0] == COV_HEAD and rep[-1] == ""
    assert rep[1] == "# TABLE_LAYOUT:  sequence " + "".join(COL + " " + c + " " for c in ref.COLUMNS) + COL + " kept"
    rows = ref.parse_report(rep[2:])
    assert len(rows) == len(rep) - 3                                            # two head lines, the rows, the empty end: no other # line
    want = {seq: (win, cov, "%.6f" % (cov / win), n, hits, "kept") for seq, (win, cov, n, hits) in table.items()}
    assert rows == want
    order = [l.split(COL)[0] for l in rep[2:-1]]
    assert order == [s for s in w["seq_col"] if s in rows]                      # ascending target id
    assert [rows[s][0] for s in order] == [w["windows"][w["seq_col"].index(s)] for s in order]


@pytest.mark.parametrize("tag,P", FIXTURES)
def test_report_behind_the_table_and_under_other_batchings(tag, P, tmp_path_factory):
    w = _world(tag, P, tmp_path_factory)
    pkg, fx, d = w["pkg"], w["fx"], w["d"]
    want = w["report"].split("\n")[:-1]
    # without FILE: the same block behind the table, in front of the summary
    r, text = _run(pkg, fx, d, ["-hits-per-seq", "-coverage"])
    lines = text.split("\n")
    i, j = _block(lines, HITS_HEAD)
    assert lines[j:j + len(want)] == want
    assert lines[j + len(want)].startswith("# queries: ")
    mask = lambda t: re.sub(r"^# (time:    |speed:   ).*$", "# T", t, flags=re.M)
    assert mask("\n".join(lines[:j] + lines[j + len(want):])) == mask(w["text"])
    # -coverage alone (no table), in small batches, and parsed by the host: the same report
    for extra in (["-coverage", "c2.txt"], ["-coverage", "c2.txt", "-batch", "16"], ["-coverage", "c2.txt", "-reader", "host"]):
        _run(pkg, fx, d, extra)
        with open(os.path.join(d, "c2.txt")) as f:
            assert f.read() == w["report"], extra
        os.remove(os.path.join(d, "c2.txt"))


@pytest.mark.parametrize("tag,P", FIXTURES)
def test_lowest_above_sequence_changes_neither_report_nor_mapping_lines(tag, P, tmp_path_factory):
    w = _world(tag, P, tmp_path_factory)
    pkg, fx, d = w["pkg"], w["fx"], w["d"]
    lowest = fx.q["lowest"]
    assert lowest != "sequence"
    _, plain = _run(pkg, fx, d, ["-tophits"], lowest=lowest)
    _, text = _run(pkg, fx, d, ["-tophits", "-coverage", "c3.txt"], lowest=lowest)
    with open(os.path.join(d, "c3.txt")) as f:
        assert f.read() == w["report"]
    maps = lambda t: [l for l in t.split("\n") if l and not l.startswith("#")]
    assert maps(text) == maps(plain) and len(maps(text)) == len(fx.names)
    head = lambda t: [l for l in t.split("\n") if l.startswith("#") and "coverage" not in l and not re.match(r"# (time|speed):", l)]
    assert head(text) == head(plain)


def test_splitout_writes_the_report_once(tmp_path_factory):
    """-splitout: the coverage is taken over all units together and written once, into FILE; a unit's output has no report"""
    w = _world("mini", 2, tmp_path_factory)
    pkg, fx, d = w["pkg"], w["fx"], w["d"]
    r = subprocess.run(_cmd(pkg, fx, ["-splitout", "-coverage", "c5.txt"]), cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    with open(os.path.join(d, "c5.txt")) as f:
        assert f.read() == w["report"]
    with open(os.path.join(d, "out.txt_r1.fq_r2.fq.txt")) as f:
        unit = f.read().split("\n")
    assert COV_HEAD not in unit and len([l for l in unit if l and not l.startswith("#")]) == len(fx.names)
    r = subprocess.run(_cmd(pkg, fx, ["-splitout", "-coverage"]), cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0 and w["report"] in r.stdout                         # without FILE: to stdout, behind the last unit's run


def _top_lists(text, name_tgt):
    """per mapping line the (target, hits) pairs of its top_hits column"""
    out = []
    for l in text.split("\n"):
        if l and not l.startswith("#"):
            col = l.split(COL)[1]
            out.append([(name_tgt[e.rsplit(":", 1)[0]], int(e.rsplit(":", 1)[1])) for e in col.split(",")] if col else [])
    return out


@pytest.mark.parametrize("tag,P", FIXTURES)
def test_cut_removes_the_least_covered_sequences_from_every_list(tag, P, tmp_path_factory):
    w = _world(tag, P, tmp_path_factory)
    pkg, fx, d = w["pkg"], w["fx"], w["d"]
    # the cut the restatement makes of part (a)'s numbers
    rows = ref.parse_report(w["report"].split("\n")[2:])
    covered = [rows[s][1] if s in rows else 0 for s in w["seq_col"]]
    removed = ref.cut(covered, w["windows"], 50)
    H = sum(1 for c in covered if c > 0)
    assert sum(removed) == H // 2 >= 1
    if tag == "tie":                                                            # 60/80 against 60/80: the exact tie, and target 0 goes
        hit = [t for t in range(fx.n_targets) if covered[t]]
        assert len(hit) == 2 and covered[hit[0]] * w["windows"][hit[1]] == covered[hit[1]] * w["windows"][hit[0]] and removed[hit[0]] == 1
    _, plain = _run(pkg, fx, d, ["-tophits"])
    r, text = _run(pkg, fx, d, ["-tophits", "-cov-percentile", "50", "-coverage", "c4.txt"])
    assert "coverage percentile 50: %d of %d hit sequences removed" % (sum(removed), H) in r.stderr
    assert "# Reference sequences below coverage percentile 50 were removed before the read mapping." in text.split("\n")
    with open(os.path.join(d, "c4.txt")) as f:
        cut_rows = ref.parse_report(f.read().split("\n")[2:])
    assert {s: v[:5] for s, v in cut_rows.items()} == {s: v[:5] for s, v in rows.items()}       # pass 1's numbers: part (a)'s
    assert {s for s, v in cut_rows.items() if v[5] == "removed"} == {w["seq_col"][t] for t in range(fx.n_targets) if removed[t]}
    assert all(v[5] in ("kept", "removed") for v in cut_rows.values())
    # the lists of pass 2: no removed sequence, and exactly the oracle's lists from the matches without those targets
    name_tgt = {s[len("sequence:"):]: t for t, s in enumerate(w["seq_col"])}
    got, before = _top_lists(text, name_tgt), _top_lists(plain, name_tgt)
    assert len(got) == len(fx.names) == len(before)
    gone = {t for t in range(fx.n_targets) if removed[t]}
    assert not any(t in gone for l in got for t, _ in l)
    keys, off, locs = dbfile.union_shards(fx.shards)
    p = fx.params
    t2t = fx.tax.target_keys(fx.n_targets, 0)
    tgt_of = {int(k): t for t, k in enumerate(t2t)}
    odb = orc.OracleDb(keys, off, locs, t2t, k=p["qk"], s=p["qs"], winlen=p["qwinlen"], winstride=p["qwinstride"], tgt_winstride=p["winstride"])
    rm = np.array(removed, bool)
    for q, (a, b) in enumerate(zip(fx.r1, fx.r2)):
        m = odb.matches(a, b)
        m = m[~rm[(m >> np.uint64(32)).astype(np.int64)]]
        c, n = odb.reduce_query(m, len(a) + len(b), max_cand=fx.maxcand, emulate_ranks=fx.P, quirk_seq_drop=1)
        want = [(tgt_of[int(tax)], int(hits)) for tax, hits, _, _ in c[:n].tolist() if hits > 0]
        assert got[q] == want, (q, fx.names[q], got[q], want)
    changed = sum(1 for x, y in zip(got, before) if x != y)
    assert changed >= 10, changed


def test_rejections_and_help(tmp_path):
    pkg = _pkg()
    fx = Fixture("mini", 2)
    _write_reads(fx, str(tmp_path))
    for extra in (["-cov-percentile", "50", "-exclude", "species"], ["-exclude", "species", "-cov-percentile", "50"], ["-cov-percentile", "101"],
                  ["-cov-percentile", "-1"], ["-cov-percentile", "x"]):
        r = subprocess.run(_cmd(pkg, fx, extra), cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
        assert r.returncode != 0, extra
        assert r.stderr.count("ABORT:") == 1 and r.stderr.count("\n") == 1 and "-cov-percentile" in r.stderr, (extra, r.stderr)
        assert not os.path.exists(tmp_path / "out.txt"), extra
    r = subprocess.run([pkg.cli_path(), "-help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert "-coverage [FILE]" in r.stdout and "-cov-percentile P" in r.stdout and "-splitout" in r.stdout.split("-coverage [FILE]")[1].split("-cov-percentile P")[0]


def test_mpi_program_rejects_both_options(tmp_path):
    pkg = _pkg()
    mpiexec = shutil.which("mpiexec") or "/opt/conda/bin/mpiexec"
    if not os.path.exists(pkg.mpi_cli_path()) or not os.path.exists(mpiexec):
        pytest.skip("no MPI on this box")
    fx = Fixture("mini", 2)
    _write_reads(fx, str(tmp_path))
    env = dict(os.environ, LD_LIBRARY_PATH=pkg.mpi_lib_dir() + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    for extra in (["-coverage"], ["-cov-percentile", "50"]):
        r = subprocess.run([mpiexec, "-n", "1", pkg.mpi_cli_path(), fx.shard_paths[0][: -len(".db_0")], "2", "r1.fq", "r2.fq"] + extra,
                           cwd=tmp_path, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
        assert r.returncode != 0
        assert "-coverage" in r.stderr and "-cov-percentile" in r.stderr and "mcq_query_cli" in r.stderr and r.stderr.count("\n") == 1
    r = subprocess.run([mpiexec, "-n", "1", pkg.mpi_cli_path(), "-help"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert "-coverage [FILE]" in r.stdout and "-cov-percentile P" in r.stdout
