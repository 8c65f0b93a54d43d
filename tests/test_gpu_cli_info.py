"""mcq_info_cli against the reference's recorded `info` output (tests/golden/info, make_golden_info.py) byte for byte, against the
restatement (tests/content_stats_ref.py, tests/bucket_limit_ref.py) where the reference has no counterpart -- the whole-database block,
-histogram, locations, the rule preview --, and its rejections."""
import functools
import gzip
import importlib
import os
import subprocess

import numpy as np
import pytest

import bucket_limit_ref
import content_stats_ref as ref
from oracle import dbfile

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
STATISTICS = [("mini", 2), ("mini", 4), ("mini", 8), ("overpop", 2), ("overpop", 4), ("noanc", 2), ("tie", 2)]
META = ["mini", "noanc", "accmap"]
STATIC_LINES = 24


def _info(tag, P, *args):
    pkg = importlib.import_module("metacache-mpi_amd")
    return subprocess.run([pkg.info_cli_path(), os.path.join(GOLDEN, tag, "P%d" % P, tag), str(P)] + [str(a) for a in args],
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)


def _ok(tag, P, *args):
    r = _info(tag, P, *args)
    assert r.returncode == 0, r.stderr
    return r.stdout


def _recorded(tag, P, r, mode):
    with gzip.open(os.path.join(GOLDEN, "info", tag, "P%d" % P, "db_%d.%s.txt.gz" % (r, mode)), "rt") as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def _shards(tag, P):
    return [dbfile.parse_shard(os.path.join(GOLDEN, tag, "P%d" % P, "%s.db_%d" % (tag, r))) for r in range(P)]


def _content(text):
    return "".join(text.splitlines(True)[STATIC_LINES:])


@pytest.mark.parametrize("tag,P", STATISTICS)
def test_statistics_of_every_shard_byte_for_byte(tag, P):
    for r in range(P):
        assert _ok(tag, P, "statistics", "-shard", r) == _recorded(tag, P, r, "statistics"), (tag, P, r)
    assert _ok(tag, P, "stat", "-shard", 0, "-chunk", 255) == _recorded(tag, P, 0, "statistics")        # (many small chunks)


@pytest.mark.parametrize("tag", META)
@pytest.mark.parametrize("mode,args", [("bare", []), ("lineages", ["lineages"]), ("rank_species", ["rank", "species"]), ("rank_genus", ["rank", "genus"])])
def test_metadata_modes_byte_for_byte(tag, mode, args):
    got = _ok(tag, 2, *args)
    for r in (0, 1):                                                         # (the taxonomy is the same in every shard)
        assert got == _recorded(tag, 2, r, mode), (tag, mode, r)


@pytest.mark.parametrize("tag", META)
@pytest.mark.parametrize("mode,args", [("targets", ["targets"]), ("targets_named", ["sequences", "NC_000003.1", "nosuchname"])])
def test_targets_with_the_owning_shards_length(tag, mode, args):
    got = _ok(tag, 2, *args).split("\n")
    rec = [_recorded(tag, 2, r, mode).split("\n") for r in (0, 1)]
    assert len(got) == len(rec[0]) == len(rec[1])
    n_len = 0
    for g, a, b in zip(got, rec[0], rec[1]):
        if a.startswith("    length: "):
            n_len += 1
            assert g.startswith("    length:     ") and g.endswith(" windows")
            assert int(g.split()[1]) == max(int(a.split()[1]), int(b.split()[1]))
        else:
            assert g == a
    assert n_len == sum(1 for l in got if l.startswith("Target ") and l.endswith("):"))            # (one length per target shown)
    if mode == "targets":
        assert n_len == _shards(tag, 2)[0]["target_count"]
        assert any(l.startswith("Target ") and l.endswith("):") for l in got)                      # (the reference's quirk)


@pytest.mark.parametrize("tag,P", [("mini", 4), ("overpop", 2), ("tie", 2)])
def test_whole_database_statistics_from_the_recorded_shards_numbers(tag, P):
    shards = _shards(tag, P)
    t = ref.zero_totals()
    for s in shards:
        t = ref.add_totals(t, ref.totals(ref.shard_features(s)))
    rec = [ref.parse_block(_recorded(tag, P, r, "statistics")) for r in range(P)]
    assert t["n_buckets"] == sum(x["features"] for x in rec) and t["max_size"] == max(x["max"] for x in rec)      # (the restatement agrees with the records)
    want = ref.content_block(*ref.meta_counts(shards[0]), sum(x["buckets"] for x in rec), sum(x["features"] for x in rec),
                             sum(x["locations"] for x in rec), t)
    got = _ok(tag, P, "statistics")
    assert got == "".join(_recorded(tag, P, 0, "statistics").splitlines(True)[:STATIC_LINES]) + want


def test_histogram_and_locations():
    shards = _shards("overpop", 2)
    t = ref.zero_totals()
    for s in shards:
        t = ref.add_totals(t, ref.totals(ref.shard_features(s)))
    got = _ok("overpop", 2, "statistics", "-histogram")
    assert got == _ok("overpop", 2, "statistics") + ref.histogram_lines(t)
    assert "bucket size 100: " in got
    one = _ok("overpop", 2, "statistics", "-histogram", "-shard", 1)
    assert one == _recorded("overpop", 2, 1, "statistics") + ref.histogram_lines(ref.totals(ref.shard_features(shards[1])))
    for tag, P in (("overpop", 2), ("mini", 4)):
        shards = _shards(tag, P)
        n = shards[0]["target_count"]
        locs = sum(ref.target_locations(s["tgt"], n) for s in shards)
        tax = {x["id"]: x for x in shards[0]["taxa"]}
        windows = [max(next(x["windows"] for x in s["taxa"] if x["id"] == -(i + 1)) for s in shards) for i in range(n)]
        names = [tax[-(i + 1)]["name"] for i in range(n)]
        assert _ok(tag, P, "locations") == ref.locations_lines(names, windows, locs, shards[0]["params"]["s"])
        assert int(locs.sum()) == sum(len(s["tgt"]) for s in shards)


@pytest.mark.parametrize("opts", [["-max-locations-per-feature", 2], ["-max-locations-per-feature", 3, "-remove-overpopulated-features"]],
                         ids=["keep_first_2", "remove_with_n_3"])
def test_statistics_under_a_bucket_rule(opts):
    shards = _shards("overpop", 2)
    limit = shards[0]["params"]["maxlocs"]
    keep_first, remove_above = bucket_limit_ref.bucket_rule(int(opts[1]), len(opts) > 2, limit)
    assert keep_first or remove_above
    plain = _ok("overpop", 2, "statistics", "-shard", 0)
    head = "".join(plain.splitlines(True)[:STATIC_LINES])
    for r in (0, 1):
        got = _ok("overpop", 2, "statistics", "-shard", r, *opts)
        assert got == head + ref.shard_block(shards[r], keep_first, remove_above)
        assert got != _recorded("overpop", 2, r, "statistics")
    # every shard together, and the per-target view of what the rule takes
    t, buckets, left = ref.zero_totals(), 0, []
    for s in shards:
        f, tg, w, _, _ = bucket_limit_ref.bucket_limit(ref.shard_features(s), s["tgt"], s["win"], keep_first, remove_above)
        t = ref.add_totals(t, ref.totals(f)); buckets += ref.reserve_buckets(len(s["keys"])); left.append(tg)
    assert _ok("overpop", 2, "statistics", *opts) == head + ref.content_block(*ref.meta_counts(shards[0]), buckets, t["n_buckets"], t["n_locations"], t)
    loc_lines = _ok("overpop", 2, "locations", *opts).split("\n")[1:-1]
    assert [int(l.split("\t")[2]) for l in loc_lines] == [int(x) for x in ref.target_locations(np.concatenate(left), shards[0]["target_count"])]


def test_a_rule_at_the_databases_own_limit_changes_nothing():
    limit = _shards("overpop", 2)[0]["params"]["maxlocs"]
    for r in (0, 1):
        assert _ok("overpop", 2, "statistics", "-shard", r, "-max-locations-per-feature", limit) == _recorded("overpop", 2, r, "statistics")


def test_featurecounts_as_sorted_lines():
    for r in (0, 1):
        got = _ok("mini", 2, "featurecounts", "-shard", r)
        want = _recorded("mini", 2, r, "featurecounts")
        assert got.count(" -> ") == len(_shards("mini", 2)[r]["keys"])
        assert sorted(got.split("\n")) == sorted(want.split("\n"))
        assert got.startswith(_recorded("mini", 2, r, "statistics") + "=" * 51 + "\n") and got.endswith("\n" + "=" * 51 + "\n")


def _rejected(r):
    assert r.returncode != 0 and r.stdout == ""
    assert sum(1 for l in r.stderr.split("\n") if l.startswith("ABORT:")) == 1, r.stderr


def test_rejections(tmp_path):
    r = _info("mini", 2, "bogus")
    _rejected(r)
    assert "Info mode 'bogus' not recognized." in r.stderr and "window stride        113" in r.stderr      # (the reference's line, the static block)
    r = _info("mini", 2, "rank")
    _rejected(r)
    assert "Please specify a taxonomic rank:" in r.stderr
    _rejected(_info("mini", 2, "statistics", "-shard", 2))
    _rejected(_info("mini", 2, "statistics", "-shard", 7))
    _rejected(_info("mini", 3, "statistics"))                                   # (mini.db_2 is not there)
    _rejected(_info("mini", 2, "featuremap"))
    pkg = importlib.import_module("metacache-mpi_amd")
    r = subprocess.run([pkg.info_cli_path(), str(tmp_path / "nothing"), "1"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    _rejected(r)
    r = subprocess.run([pkg.info_cli_path(), "-help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    for word in ("targets", "lineages", "rank RANK", "statistics", "locations", "featurecounts", "-shard", "-histogram", "-max-locations-per-feature",
                 "-remove-overpopulated-features", "-device", "-chunk", "featuremap", "hash"):
        assert word in r.stdout, word
