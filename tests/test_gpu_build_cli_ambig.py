"""mcq_build_cli -remove-ambig-features RANK [-max-ambig-per-feature N]: a fresh child process per build, as
tests/test_gpu_build_cli.py starts it.  The reference's MPI build accepts the options and ignores them, so there is no golden file:
the expectation is the same build without the options, filtered by the NumPy statement of remove_ambiguous_features
(tests/ambig_ref.py) over the triples of all rank files together.  The counts in CASES were computed on the CPU from the golden
shards with that filter."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import ambig_ref as ar
import build_inputs as bi
from golden_util import Fixture
from oracle import dbfile
from oracle import mc_oracle as orc

pytestmark = pytest.mark.gpu

RANKS = {"sequence": 0, "species": 4, "genus": 6, "family": 10}
AMBIG = "-remove-ambig-features"
# (fixture, P, options besides the fixture's own, rank, N as the program takes it, (removed, keys) or None: whatever the filter gives)
CASES = [(tag, P, opts, rank, n, want)
         for P in (2, 8)
         for tag, opts, rank, n, want in (("mini", [AMBIG, "species"], "species", 1, (798, 11327)),
                                          ("mini", [AMBIG, "species", "-max-ambig-per-feature", "2"], "species", 2, (182, 11327)),
                                          ("mini", [AMBIG, "sequence", "-max-ambig-per-feature", "258"], "sequence", 2, (1857, 11327)))] + [
    ("noanc", 2, [AMBIG, "species"], "species", 1, (921, 3623)),
    ("tie", 4, [AMBIG, "species"], "species", 1, (1280, 1280)),
    ("tie", 4, ["-remove_ambig_features", "genus", "-max_ambig_per_feature", "2"], "genus", 2, (0, 1280)),
    ("tie", 4, [AMBIG, "family"], "family", 1, (0, 1280)),            # four targets without a family: "none" is one value
    ("overpop", 2, [AMBIG, "species"], "species", 1, (17, 3233)),     # (-remove-overpopulated-features is the fixture's own option: it comes first)
    ("wide", 16, [AMBIG, "species"], "species", 1, None)]


@pytest.fixture(scope="module")
def mods():
    pkg = importlib.import_module("metacache-mpi_amd")
    pkg.build_host()
    return pkg, importlib.import_module("metacache-mpi_amd.host")


def _build(pkg, work, name, P, extra=(), timeout=600):
    return subprocess.run([pkg.build_cli_path(), name, str(P), "genomes", "-taxonomy", "tax"] + list(extra), cwd=work,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)


def _rank_file(host, work, name, rank, tag):
    """one rank's file alone, as <work>/<tag>/x.db_0 -> (info without the table's counts, taxon list, (feature, target, window) rows)"""
    d = os.path.join(work, tag)
    os.makedirs(d)
    os.symlink(os.path.join(work, "%s.db_%d" % (name, rank)), os.path.join(d, "x.db_0"))
    db = host.RefDb(os.path.join(d, "x"), 1, meta_only=True)
    info = {f: getattr(db.info, f) for f, _ in host.Info._fields_ if f not in ("n_keys", "n_locs")}
    chunks = list(db.stream(0, chunk=1 << 16))
    tri = np.concatenate([np.stack(c, axis=1) for c in chunks]) if chunks else np.zeros((0, 3), np.uint32)
    return info, bi.taxon_list(db), tri


def _sorted(tri):
    return tri[np.lexsort((tri[:, 2], tri[:, 1], tri[:, 0]))]


_plain = {}


@pytest.fixture(scope="module")
def plain(mods, tmp_path_factory):
    """the build of a fixture at P without the option, made once: (work directory, per rank (info, taxa, triples), stdout)"""
    pkg, host = mods

    def get(tag, P):
        if (tag, P) not in _plain:
            work = bi.lay_out(tag, str(tmp_path_factory.mktemp("%s_P%d" % (tag, P)) / "w"))
            r = _build(pkg, work, "plain", P, bi.FIXTURES[tag][1])
            assert r.returncode == 0, r.stderr[-2000:]
            assert "ambiguous features" not in r.stdout
            _plain[(tag, P)] = (work, [_rank_file(host, work, "plain", rank, "plain%d" % rank) for rank in range(P)], r.stdout)
        return _plain[(tag, P)]
    yield get
    _plain.clear()


def _tgt_key(host, work, P, rank):
    db = host.RefDb(os.path.join(work, "plain"), P, meta_only=True)
    return np.arange(db.info.n_targets, dtype=np.uint32) if rank == "sequence" else db.clade_keys(RANKS[rank])


@pytest.mark.parametrize("tag,P,opts,rank,n,want", CASES, ids=["%s-P%d-%s" % (c[0], c[1], "_".join(o.strip("-") for o in c[2][1:])) for c in CASES])
def test_files_hold_the_filtered_build(mods, plain, tag, P, opts, rank, n, want):
    pkg, host = mods
    work, base, _ = plain(tag, P)
    name = "amb_" + "_".join(o.strip("-").replace("-", "").replace("_", "") for o in opts)
    r = _build(pkg, work, name, P, bi.FIXTURES[tag][1] + opts)
    assert r.returncode == 0, r.stderr[-2000:]
    mine = [_rank_file(host, work, name, rank_, "%s_%d" % (name, rank_)) for rank_ in range(P)]
    all_plain = np.concatenate([b[2] for b in base])
    expect, removed, n_keys = ar.filter_triples(all_plain, _tgt_key(host, work, P, rank), n)
    if want is not None:
        assert (removed, n_keys) == want
    got = np.concatenate([m[2] for m in mine])
    assert got.shape == expect.shape and np.array_equal(_sorted(got), _sorted(expect))
    for rank_ in range(P):
        assert (mine[rank_][2][:, 1] % P == rank_).all()
        assert mine[rank_][0] == base[rank_][0] and mine[rank_][1] == base[rank_][1], rank_       # parameters, taxa, `windows`
    a = host.RefDb(os.path.join(work, name), P, meta_only=True)
    b = host.RefDb(os.path.join(work, "plain"), P, meta_only=True)
    assert np.array_equal(a.tgt_windows(), b.tgt_windows())
    line = "ambiguous features on rank %s (more than %d taxa): %d of %d removed" % (rank, n, removed, n_keys)
    out = r.stdout.strip().split("\n")
    keys_in_files = sum(len(np.unique(m[2][:, 0])) for m in mine)
    assert len(out) >= 2 and out[-2] == line and out[-1].endswith(": %d keys, %d locations" % (keys_in_files, len(got))), r.stdout


def _write_reads(fx, work):
    for fn, seqs in (("r1.fq", fx.r1), ("r2.fq", fx.r2)):
        with open(os.path.join(work, fn), "w") as f:
            for nm, s in zip(fx.names, seqs):
                f.write("@%s\n%s\n+\n%s\n" % (nm, s, "I" * len(s)))


def _query(pkg, fx, work, name, P, out):
    q = subprocess.run([pkg.cli_path(), name, str(P), "r1.fq", "r2.fq", "-lowest", fx.q["lowest"], "-maxcand", str(fx.maxcand), "-hitmin", str(fx.hitmin),
                        "-hitdiff", str(fx.q["hitdiff"]), "-threads", "2", "-out", out], cwd=work, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=600)
    assert q.returncode == 0, q.stderr[-2000:]
    text = open(os.path.join(work, out)).read()
    return text, [l.split("\t|\t") for l in text.split("\n") if "\t|\t" in l and not l.startswith("#")]


def test_a_build_that_removes_every_feature_writes_files_that_open_and_query(mods, plain):
    """tie at species: every feature is shared by two species; the four files hold no key, the host library opens them and
    mcq_query_cli classifies nothing"""
    pkg, host = mods
    work, _, _ = plain("tie", 4)
    r = _build(pkg, work, "empty", 4, [AMBIG, "species"])
    assert r.returncode == 0 and "1280 of 1280 removed" in r.stdout, (r.stdout, r.stderr[-2000:])
    db = host.RefDb(os.path.join(work, "empty"), 4)
    assert db.info.n_keys == 0 and db.info.n_locs == 0 and db.info.n_targets == 4
    meta = host.RefDb(os.path.join(work, "empty"), 4, meta_only=True)
    assert all(meta.file_stats(rank)[1:] == (0, 0) for rank in range(4))
    fx = Fixture("tie", 4)
    _write_reads(fx, work)
    text, lines = _query(pkg, fx, work, "empty", 4, "empty.txt")
    assert len(lines) == len(fx.names) and all(l[1] == "--" for l in lines), lines[:3]
    assert "None of the input sequences could be classified." in text


def test_an_unknown_rank_builds_the_unfiltered_database_with_a_warning(mods, plain):
    pkg, host = mods
    work, base, stdout = plain("noanc", 2)
    for i, word in enumerate(("nosuchrank", "none")):
        r = _build(pkg, work, "unk%d" % i, 2, [AMBIG, word, "-max-ambig-per-feature", "3"])
        assert r.returncode == 0, r.stderr[-2000:]
        warnings = [l for l in r.stderr.split("\n") if l.startswith("warning:")]
        assert len(warnings) == 1 and word in warnings[0], r.stderr
        assert "ambiguous features" not in r.stdout and r.stdout.replace("unk%d" % i, "plain") == stdout
        for rank in range(2):
            info, taxa, tri = _rank_file(host, work, "unk%d" % i, rank, "unk%d_%d" % (i, rank))
            assert info == base[rank][0] and taxa == base[rank][1] and np.array_equal(tri, base[rank][2])


def test_help_names_both_options_and_the_divergence(mods):
    pkg, host = mods
    r = subprocess.run([pkg.build_cli_path(), "-help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    text = " ".join(r.stdout.split())
    assert "-remove-ambig-features RANK" in text and "-max-ambig-per-feature N" in text
    assert "the reference's `mpiexec -n P metacache_mpi build` accepts the options and ignores them" in text
    src = open(os.path.join(os.path.dirname(pkg.build_cli_path()), "csrc", "host", "mcq_build_cli.cpp")).read()
    head = " ".join(l.lstrip("/ ") for l in src[:src.index("#include")].split("\n"))
    assert "the reference's `mpiexec -n P metacache_mpi build` accepts the options and ignores them" in " ".join(head.split())
    r = subprocess.run([pkg.build_cli_path(), "x", "2", "genomes", "-taxonomy", "tax", "-no-such-option"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=60)
    assert r.returncode != 0 and "ABORT: unknown option" in r.stderr


def test_query_cli_on_a_filtered_build_classifies_like_the_oracle_on_the_filtered_table(mods, plain):
    """mini at P = 4, species, N = 1: the mapping lines of mcq_query_cli on the built files, per read header, against the oracle's
    candidates on the NumPy-filtered union of the golden shards, classified by the host library"""
    pkg, host = mods
    fx, P = Fixture("mini", 4), 4
    work, _, _ = plain("mini", 4)
    r = _build(pkg, work, "filtered", P, [AMBIG, "species"])
    assert r.returncode == 0 and "798 of 11327 removed" in r.stdout, (r.stdout, r.stderr[-2000:])
    _write_reads(fx, work)
    _, lines = _query(pkg, fx, work, "filtered", P, "filtered.txt")
    rdb = host.RefDb(fx.shard_paths[0][: -len(".db_0")], P)
    keys, off, locs = dbfile.union_shards(fx.shards)
    fk, fo, fl, removed = ar.numpy_filter(keys, off, locs, rdb.clade_keys(RANKS["species"]), 1)
    assert removed == 798
    p = fx.params
    odb = orc.OracleDb(fk, fo, fl, rdb.tgt2tax(fx.lowest), k=p["qk"], s=p["qs"], winlen=p["qwinlen"], winstride=p["qwinstride"], tgt_winstride=p["winstride"])
    bases, seq_off = orc.pack_reads(fx.interleaved())
    cand, ncand = odb.query(bases, seq_off, True, max_cand=fx.maxcand, emulate_ranks=P, quirk_seq_drop=1)
    want = []
    for q, name in enumerate(fx.names):
        best = rdb.classify(cand[q, :ncand[q]], fx.hitmin, fx.hitdiff, fx.highest)
        want.append([name, "--" if best == host.NO_TAXON else "%s:%s" % (host.lib().mcq_rank_name(rdb.taxon_rank(best)).decode(), rdb.taxon_name(best))])
    assert sorted(lines) == sorted(want)
    assert sum(1 for w in want if w[1] != "--") > 150 and len(want) == 197
