"""-queryids, -locations and -allhits through mcq_query_cli (fresh child processes, as tests/test_gpu_cli.py starts them).

The expected -out files are built from the committed goldens of the reference (tests/golden/*/P*/cli_*.out.gz) plus the
restatement of the new columns (tests/all_hits_ref.py over OracleDb.matches / OracleDb.query).  The whole file is compared after
sorting, the measured values of "# time:" and "# speed:" masked, as that test does."""
import gzip
import importlib
import json
import os
import re
import shutil
import subprocess

import pytest

import all_hits_ref as ahr
import build_inputs as bi
from golden_util import GOLDEN, Fixture
from oracle import dbfile
from oracle import mc_oracle as orc

pytestmark = pytest.mark.gpu
COL = "\t|\t"
LAYOUT = "# TABLE_LAYOUT: "
SEQ_OPTS = ["-lowest", "sequence", "-threads", "2", "-maxcand", "4", "-hitmin", "4", "-hitdiff", "80"]      # of cli_seq_plain.out.gz


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


def fixture_opts(fx):
    return ["-lowest", fx.q["lowest"], "-maxcand", str(fx.maxcand), "-hitmin", str(fx.hitmin), "-hitdiff", str(fx.q["hitdiff"]), "-threads", "2"]


_runs = {}


def run_cli(tmp_path_factory, tag, P, opts, headers=None, prefix=None, pre=()):
    """(return code, -out text, stderr) of one run in a working directory of its own; each distinct run is made once per module"""
    key = (tag, P, tuple(opts), headers is not None, prefix, tuple(pre))
    if key not in _runs:
        pkg = _pkg()
        fx = Fixture(tag, P if prefix is None else 2)
        cwd = tmp_path_factory.mktemp("cli_allhits")
        for fn, seqs in (("r1.fq", fx.r1), ("r2.fq", fx.r2)):
            with open(cwd / fn, "w") as f:
                for n, s in zip(headers or fx.names, seqs):
                    f.write("@%s\n%s\n+\n%s\n" % (n, s, "I" * len(s)))
        r = subprocess.run([pkg.cli_path(), prefix or fx.shard_paths[0][: -len(".db_0")], str(P), "r1.fq", "r2.fq"] + list(pre) + list(opts) +
                           ["-out", "out.txt"], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
        _runs[key] = (r.returncode, open(cwd / "out.txt").read() if os.path.exists(cwd / "out.txt") else "", r.stderr)
    return _runs[key]


def rebuilt(ref, has_top, ids=None, allcol=None, locs=None):
    """the reference's file `ref` with the new columns put in: ids {name: number}, allcol {name: text}, locs(columns of the line) -> text"""
    out = []
    for l in ref.split("\n"):
        if l.startswith(LAYOUT):
            c = l[len(LAYOUT):].split(COL)
            l = LAYOUT + COL.join((["query_id"] if ids else []) + [c[0]] + (["all_hits"] if allcol is not None else []) + (c[1:2] if has_top else []) +
                                  (["candidate_locations"] if locs else []) + [c[-1]])
        elif l and not l.startswith("#"):
            c = l.split(COL)
            assert len(c) == (3 if has_top else 2), l
            l = COL.join(([str(ids[c[0]])] if ids else []) + [c[0]] + ([allcol[c[0]]] if allcol is not None else []) + (c[1:2] if has_top else []) +
                         ([locs(c)] if locs else []) + [c[-1]])
        out.append(l)
    return "\n".join(out)


_worlds = {}


def all_hits_of(tag, P, lowest):
    """(fixture, per read its entries from the oracle on the union table, {target: the name printed at rank `lowest`}, whether that
    rank is `sequence`)"""
    key = (tag, P)
    if key not in _worlds:
        fx = Fixture(tag, P)
        keys, off, locs = dbfile.union_shards(fx.shards)
        p = fx.params
        odb = orc.OracleDb(keys, off, locs, fx.tax.target_keys(fx.n_targets, 0), k=p["qk"], s=p["qs"], winlen=p["qwinlen"],
                           winstride=p["qwinstride"], tgt_winstride=p["winstride"])
        _worlds[key] = (fx, [ahr.rle(odb.matches(a, b)) for a, b in zip(fx.r1, fx.r2)])
    fx, ent = _worlds[key]
    li = dbfile.RANK_NAMES.index(lowest)
    tnames = {t: ahr.name_of_target(fx.tax, t, li) for t in range(fx.n_targets)}
    return fx, ent, tnames, li == 0


# ---- -queryids -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alias", ["-queryids", "-query_id"])
def test_queryids(alias, tmp_path_factory):
    fx = Fixture("mini", 4)
    rc, mine, err = run_cli(tmp_path_factory, "mini", 4, fixture_opts(fx) + [alias])
    assert rc == 0, err
    ids = {n: i + 1 for i, n in enumerate(fx.names)}
    want = rebuilt(golden(fx, "cli_default.out.gz"), False, ids=ids)
    assert LAYOUT + "query_id" + COL + "query_header" + COL in want
    assert norm(mine) == norm(want)


# ---- -locations ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,P", [("mini", 4), ("tie", 2)])
def test_locations_after_a_fold(tag, P, tmp_path_factory):
    """n_ranks > 1: the folded candidates carry (0,0), every entry is [0,<winlen>] -- what the reference's MPI program prints"""
    fx = Fixture(tag, P)
    rc, mine, err = run_cli(tmp_path_factory, tag, P, fixture_opts(fx) + ["-tophits", "-locations"])
    assert rc == 0, err
    assert fx.params["winlen"] == 128
    want = rebuilt(golden(fx, "cli_tophits.out.gz"), True, locs=lambda c: "[0,128] " * len([t for t in c[1].split(",") if t]))
    assert LAYOUT + "query_header" + COL + "top_hits" + COL + "candidate_locations" + COL in want and "[0,128] [0,128] " in want
    assert norm(mine) == norm(want)


def test_locations_of_a_one_rank_database(tmp_path_factory):
    """a database of one rank, built from the fixture's genomes by mcq_build_cli: the real ranges, against OracleDb.query"""
    pkg = _pkg()
    fx = Fixture("mini", 2)
    work = bi.lay_out("mini", str(tmp_path_factory.mktemp("one_rank") / "w"))
    b = subprocess.run([pkg.build_cli_path(), "mini", "1", "genomes", "-taxonomy", "tax"], cwd=work, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-2000:]
    rc, mine, err = run_cli(tmp_path_factory, "mini", 1, fixture_opts(fx) + ["-tophits", "-locations"], prefix=os.path.join(work, "mini"))
    assert rc == 0, err
    shard = dbfile.parse_shard(os.path.join(work, "mini.db_0"))
    keys, off, locs = dbfile.union_shards([shard])
    tax = dbfile.Taxonomy(shard["taxa"])
    p = shard["params"]
    odb = orc.OracleDb(keys, off, locs, tax.target_keys(shard["target_count"], fx.lowest), k=p["qk"], s=p["qs"], winlen=p["qwinlen"],
                       winstride=p["qwinstride"], tgt_winstride=p["winstride"])
    rb, ro = orc.pack_reads(fx.interleaved())
    cand, ncand = odb.query(rb, ro, True, max_cand=fx.maxcand, emulate_ranks=1, quirk_seq_drop=1)
    rows = {l.split(COL)[0]: l.split(COL) for l in mine.split("\n") if l and not l.startswith("#")}
    assert len(rows) == len(fx.names)
    moved = 0
    for q, name in enumerate(fx.names):
        c = [x for x in cand[q, :ncand[q]].tolist() if x[1] > 0]
        want = ahr.locations_column([(x[2], x[3]) for x in c], p["winstride"], p["winlen"])
        assert len(rows[name]) == 4 and rows[name][2] == want, (name, rows[name], want)
        assert len([t for t in rows[name][1].split(",") if t]) == len(c), name
        moved += any(x[2] > 0 for x in c)
    assert moved > len(fx.names) // 2                           # real positions, not the fold's zeros


# ---- -allhits --------------------------------------------------------------------------------------------------------------------
def test_allhits_at_sequence_level(tmp_path_factory):
    fx, ent, tnames, seq = all_hits_of("mini", 4, "sequence")
    rc, mine, err = run_cli(tmp_path_factory, "mini", 4, SEQ_OPTS + ["-allhits"])
    assert rc == 0, err
    col = {n: ahr.all_hits_column(e, tnames, True) for n, e in zip(fx.names, ent)}
    assert seq and sum(c != "" for c in col.values()) > 100 and "" in col.values()
    want = rebuilt(golden(fx, "cli_seq_plain.out.gz"), False, allcol=col)
    assert LAYOUT + "query_header" + COL + "all_hits" + COL in want
    assert norm(mine) == norm(want)


@pytest.mark.parametrize("tag,P", [("mini", 4), ("tie", 2)])
def test_allhits_at_the_fixtures_rank(tag, P, tmp_path_factory):
    fx, ent, tnames, seq = all_hits_of(tag, P, Fixture(tag, P).q["lowest"])
    rc, mine, err = run_cli(tmp_path_factory, tag, P, fixture_opts(fx) + ["-all-hits"])
    assert rc == 0, err
    col = {n: ahr.all_hits_column(e, tnames, False) for n, e in zip(fx.names, ent)}
    assert not seq
    assert norm(mine) == norm(rebuilt(golden(fx, "cli_default.out.gz"), False, allcol=col))


def test_all_three_columns_in_order(tmp_path_factory):
    fx, ent, tnames, seq = all_hits_of("mini", 4, "species")
    rc, mine, err = run_cli(tmp_path_factory, "mini", 4, fixture_opts(fx) + ["-allhits", "-tophits", "-locations", "-queryids"])
    assert rc == 0, err
    col = {n: ahr.all_hits_column(e, tnames, False) for n, e in zip(fx.names, ent)}
    want = rebuilt(golden(fx, "cli_tophits.out.gz"), True, ids={n: i + 1 for i, n in enumerate(fx.names)}, allcol=col,
                   locs=lambda c: "[0,128] " * len([t for t in c[1].split(",") if t]))
    assert LAYOUT + COL.join(["query_id", "query_header", "all_hits", "top_hits", "candidate_locations", "rank:taxname"]) in want.split("\n")
    assert norm(mine) == norm(want)


def test_map_view_mode(tmp_path_factory):
    fx = Fixture("mini", 4)
    rc, base, err = run_cli(tmp_path_factory, "mini", 4, fixture_opts(fx) + ["-all-hits"])
    assert rc == 0, err
    unmapped = [l for l in base.split("\n") if l and not l.startswith("#") and l.endswith(COL + "--")]
    assert unmapped                                             # the fixture has reads without a classification
    for pre in (["-mapped-only"], ["-nomap"]):                  # -allhits shows every read
        rc, mine, err = run_cli(tmp_path_factory, "mini", 4, fixture_opts(fx) + ["-all-hits"], pre=pre)
        assert rc == 0, err
        assert norm(mine) == norm(base), pre
    # ... unless -nomap -tophits has already made it `mapped-only`
    rc, both, err = run_cli(tmp_path_factory, "mini", 4, fixture_opts(fx) + ["-allhits", "-tophits"])
    assert rc == 0, err
    rc, mo, err = run_cli(tmp_path_factory, "mini", 4, fixture_opts(fx) + ["-allhits"], pre=["-nomap", "-tophits"])
    assert rc == 0, err
    assert mo.split("\n")[0] == "# Reporting per-read mappings (non-mapping lines start with '# ')."
    assert "# Per-Read mappings will not be shown." not in mo
    keep = [l for l in both.split("\n") if l.startswith("#") or not l.endswith(COL + "--")]
    assert norm(mo) == norm("\n".join(keep)) and len(keep) < len(both.split("\n"))


def test_allhits_under_exclusion(tmp_path_factory):
    """-exclude species: the entries on targets of the read's own species are left out; the rest of the file is the reference's"""
    host = importlib.import_module("metacache-mpi_amd.host")
    fx, ent, tnames, seq = all_hits_of("mini", 4, "species")
    with open(os.path.join(GOLDEN, "mini", "eval_headers.json")) as f:
        headers = json.load(f)
    opts = ["-pairfiles", "-lowest", fx.q["lowest"], "-threads", "2", "-maxcand", str(fx.maxcand), "-hitmin", "4", "-hitdiff", "80",
            "-exclude", "species"]                              # (the run that made cli_excl_species.out.gz)
    rc, mine, err = run_cli(tmp_path_factory, "mini", 4, opts + ["-allhits"], headers=headers)
    assert rc == 0, err
    rdb = host.RefDb(fx.shard_paths[0][: -len(".db_0")], 4)
    sp = dbfile.RANK_NAMES.index("species")
    tclade = rdb.clade_keys(sp)
    col, dropped = {}, 0
    for h, e in zip(headers, ent):
        qc = rdb.taxon_clade(rdb.ground_truth(h), sp)
        drop = {t for t in range(fx.n_targets) if int(tclade[t]) == qc}
        dropped += any(int(t) in drop for t in e["tgt"])
        col[h.split(" ")[0]] = ahr.all_hits_column(e, tnames, False, drop=drop)
    assert dropped > 50
    assert norm(mine) == norm(rebuilt(golden(fx, "cli_excl_species.out.gz"), False, allcol=col))


def test_batches_and_threads_do_not_matter(tmp_path_factory):
    fx = Fixture("mini", 4)
    opts = ["-lowest", fx.q["lowest"], "-maxcand", str(fx.maxcand), "-hitmin", str(fx.hitmin), "-hitdiff", str(fx.q["hitdiff"])]
    rc, base, err = run_cli(tmp_path_factory, "mini", 4, opts + ["-threads", "2", "-allhits", "-tophits", "-locations", "-queryids"])
    assert rc == 0, err
    rc, mine, err = run_cli(tmp_path_factory, "mini", 4, opts + ["-threads", "3", "-batch", "7", "-allhits", "-tophits", "-locations", "-queryids"])
    assert rc == 0, err
    assert norm(mine.replace("# Using 3 threads", "# Using 2 threads")) == norm(base)


def test_help_names_the_options():
    h = subprocess.run([_pkg().cli_path(), "-help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    for word in ("-queryids", "-locations", "-allhits", "mcq_query_mpi rejects it and names mcq_query_cli; alias -all-hits"):
        assert word in h.stdout, word


def test_mpi_program_rejects_allhits(tmp_path):
    """mcq_query_mpi shares the parser: it names mcq_query_cli and leaves before it opens a GPU or the database"""
    pkg = _pkg()
    mpiexec = shutil.which("mpiexec") or "/opt/conda/bin/mpiexec"
    if not os.path.exists(pkg.mpi_cli_path()) or not os.path.exists(mpiexec):
        pytest.skip("no MPI on this box")
    env = dict(os.environ, LD_LIBRARY_PATH=pkg.mpi_lib_dir() + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    for opt in (["-allhits"], ["-all-hits", "-queryids"]):
        r = subprocess.run([mpiexec, "-n", "1", pkg.mpi_cli_path(), str(tmp_path / "no_such_db"), "4", "r1.fq", "r2.fq"] + opt,
                           cwd=tmp_path, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
        assert r.returncode != 0, opt
        assert "-allhits is an option of mcq_query_cli" in r.stderr and "no_such_db" not in r.stderr, (opt, r.stderr)


def test_mpi_program_writes_query_ids_and_locations(tmp_path):
    """-queryids and -locations come to mcq_query_mpi through the shared parser and writer: two ranks on one GPU (-transport mpi)
    write the reference's -tophits file with the two columns put in"""
    pkg = _pkg()
    mpiexec = shutil.which("mpiexec") or "/opt/conda/bin/mpiexec"
    if not os.path.exists(pkg.mpi_cli_path()) or not os.path.exists(mpiexec):
        pytest.skip("no MPI on this box")
    fx = Fixture("mini", 4)
    for fn, seqs in (("r1.fq", fx.r1), ("r2.fq", fx.r2)):
        with open(tmp_path / fn, "w") as f:
            for n, s in zip(fx.names, seqs):
                f.write("@%s\n%s\n+\n%s\n" % (n, s, "I" * len(s)))
    env = dict(os.environ, LD_LIBRARY_PATH=pkg.mpi_lib_dir() + ":" + os.environ.get("LD_LIBRARY_PATH", ""), HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([mpiexec, "-n", "2", pkg.mpi_cli_path(), fx.shard_paths[0][: -len(".db_0")], "4", "r1.fq", "r2.fq"] + fixture_opts(fx) +
                       ["-tophits", "-locations", "-query-ids", "-batch", "40", "-transport", "mpi", "-out", "out.txt"],
                       cwd=tmp_path, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    want = rebuilt(golden(fx, "cli_tophits.out.gz"), True, ids={n: i + 1 for i, n in enumerate(fx.names)},
                   locs=lambda c: "[0,128] " * len([t for t in c[1].split(",") if t]))
    assert norm(open(tmp_path / "out.txt").read()) == norm(want)


def test_batches_without_any_hit(tmp_path):
    """reads that hit nothing: an empty all_hits column, whether such reads fill whole batches (the first batch of every slot here)
    or the whole input"""
    import numpy as np
    pkg = _pkg()
    fx, ent, tnames, seq = all_hits_of("mini", 4, "species")
    keys, off, locs = dbfile.union_shards(fx.shards)
    p = fx.params
    odb = orc.OracleDb(keys, off, locs, fx.tgt2tax(), k=p["qk"], s=p["qs"], winlen=p["qwinlen"], winstride=p["qwinstride"],
                       tgt_winstride=p["winstride"])
    rng = np.random.default_rng(5)
    rnd = [("rnd%02d" % i, "".join(rng.choice(list("ACGT"), 150)), "".join(rng.choice(list("ACGT"), 150))) for i in range(12)]
    rnd.append(("short", "ACGTACG", "ACGTA"))                     # shorter than k
    assert all(len(odb.matches(a, b)) == 0 for _, a, b in rnd)
    empty = [n + COL + COL + "--" for n, _, _ in rnd]
    col = {n: ahr.all_hits_column(e, tnames, False) for n, e in zip(fx.names, ent)}
    ref = [l for l in rebuilt(golden(fx, "cli_default.out.gz"), False, allcol=col).split("\n") if l and not l.startswith("#")]
    prefix = fx.shard_paths[0][: -len(".db_0")]
    for name, reads, want in (("only", rnd, empty), ("first", rnd + list(zip(fx.names, fx.r1, fx.r2)), empty + ref)):
        for fn, k in (("r1.fq", 1), ("r2.fq", 2)):
            with open(tmp_path / fn, "w") as f:
                for r in reads:
                    f.write("@%s\n%s\n+\n%s\n" % (r[0], r[k], "I" * len(r[k])))
        r = subprocess.run([pkg.cli_path(), prefix, "4", "r1.fq", "r2.fq"] + fixture_opts(fx) + ["-batch", "4", "-allhits", "-out", name + ".txt"],
                           cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
        assert r.returncode == 0, (name, r.stderr)
        lines = open(tmp_path / (name + ".txt")).read().split("\n")
        assert LAYOUT + COL.join(["query_header", "all_hits", "rank:taxname"]) in lines
        assert sorted(l for l in lines if COL in l and not l.startswith("#")) == sorted(want), name      # (the mapping lines: the summary of a
        # run without a classified read has a line of plain text)
