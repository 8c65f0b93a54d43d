"""tests/content_stats_ref.py against the reference's recorded `info <db>.db_<r> statistics` output (tests/golden/info,
make_golden_info.py): the content block -- the float bucket arithmetic, the moment formulas, the number format -- text for text
from the shard files as oracle/dbfile.parse_shard reads them, and the whole-database block from the shards' summed totals."""
import gzip
import os

import numpy as np
import pytest

import content_stats_ref as ref
from oracle import dbfile

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
STATISTICS = [("mini", 2), ("mini", 4), ("mini", 8), ("overpop", 2), ("overpop", 4), ("noanc", 2), ("tie", 2)]
STATIC_LINES = 24           # print_static_properties writes 24 lines; the content block follows


def recorded(tag, P, r, mode="statistics"):
    with gzip.open(os.path.join(GOLDEN, "info", tag, "P%d" % P, "db_%d.%s.txt.gz" % (r, mode)), "rt") as f:
        return f.read()


def content_of(text):
    return "".join(text.splitlines(True)[STATIC_LINES:])


def shard(tag, P, r):
    return dbfile.parse_shard(os.path.join(GOLDEN, tag, "P%d" % P, "%s.db_%d" % (tag, r)))


@pytest.mark.parametrize("tag,P", STATISTICS)
def test_content_block_of_every_recorded_shard(tag, P):
    for r in range(P):
        want = content_of(recorded(tag, P, r))
        assert want.startswith("targets ") and "bucket size " in want
        assert ref.shard_block(shard(tag, P, r)) == want, (tag, P, r)


def test_static_block_is_the_same_text_in_every_fixture_with_these_parameters():
    head = "".join(recorded("mini", 2, 0).splitlines(True)[:STATIC_LINES])
    assert head.count("------------------------------------------------\n") == 6
    for tag, P in STATISTICS:
        for r in range(P):
            assert recorded(tag, P, r).startswith(head)
    assert recorded("mini", 2, 1, "bare").startswith(head)


@pytest.mark.parametrize("tag,P", STATISTICS)
def test_whole_database_block_is_the_block_of_the_summed_totals(tag, P):
    shards = [shard(tag, P, r) for r in range(P)]
    t, buckets = ref.zero_totals(), 0
    for s in shards:
        t = ref.add_totals(t, ref.totals(ref.shard_features(s)))
        buckets += ref.reserve_buckets(len(s["keys"]))
    # the same from every bucket of every shard at once, and from the recorded blocks' own numbers
    lengths = np.concatenate([np.diff(s["off"].astype(np.int64)) for s in shards])
    assert ref.same_totals(t, ref.totals_of_lengths(lengths))
    rec = [ref.parse_block(recorded(tag, P, r)) for r in range(P)]
    assert buckets == sum(x["buckets"] for x in rec)
    assert t["n_buckets"] == sum(x["features"] for x in rec) and t["n_locations"] == sum(x["locations"] for x in rec)
    assert t["max_size"] == max(x["max"] for x in rec)
    block = ref.content_block(*ref.meta_counts(shards[0]), buckets, t["n_buckets"], t["n_locations"], t)
    assert ("features             %d\n" % sum(x["features"] for x in rec)) in block
    assert ("buckets              %d\n" % buckets) in block


def test_totals_and_histogram_of_small_inputs():
    t = ref.totals([7, 7, 7, 9, 7, 7])                     # equal features in two runs that do not touch: two buckets
    assert (t["n_buckets"], t["n_locations"], t["sum2"], t["sum3"], t["max_size"]) == (3, 6, 14, 36, 3)
    assert t["hist"][1] == 1 and t["hist"][2] == 1 and t["hist"][3] == 1 and t["hist"].sum() == 3
    t = ref.totals(np.repeat(np.arange(4, dtype=np.uint32), [254, 255, 256, 300]))
    assert t["hist"][254] == 1 and t["hist"][255] == 3 and t["max_size"] == 300 and t["hist"][0] == 0
    assert ref.totals([])["n_buckets"] == 0
    assert ref.histogram_lines(ref.totals([1, 2, 2])) == "bucket size 1: 1\nbucket size 2: 1\n"
    assert np.array_equal(ref.target_locations([0, 2, 2], 4), [1, 0, 2, 0])


def test_number_format_and_degenerate_moments():
    assert ref.cout_double(254.0) == "254" and ref.cout_double(1.0455550) == "1.04556" and ref.cout_double(1234567.0) == "1.23457e+06"
    mx, mean, sd, skew = ref.moments(ref.totals([5]))                                                       # one bucket: 0 / 0 in the variance
    assert (mx, mean, skew) == (1.0, 1.0, 0.0) and np.isnan(sd)
    mx, mean, sd, skew = ref.moments(ref.totals([1, 1, 2, 2, 3, 3]))                                        # all sizes equal: 0 / 0 in the skewness
    assert (mx, mean, sd) == (2.0, 2.0, 0.0) and ref.cout_double(skew) == "-nan"
    assert ref.reserve_buckets(8144) == 10181 and ref.reserve_buckets(1280) == 1601
