"""A NumPy statement of the content statistics: what mcq_content_stats_* gathers over chunks of
(feature, target, window) triples, and the text `metacache_mpi info DB statistics` makes of it.

A maximal run of equal `feat` is one bucket (the chunk holds whole key records of one shard file).  Totals are exact integers:
buckets, locations, the sums of size^2 and size^3, the largest size, hist[s] = buckets of s locations with hist[255] = 255 and more.
The text restates print_content_properties (src/sketch_database.h:1205-1237): `buckets` is hash_multimap::reserve_keys
(src/hash_multimap.h:611-613) in float as it is written, `bucket size` the statistics_accumulator's max / mean / stddev / skewness
(src/stat_combined.h, src/stat_moments.h:565-572, :680-696, :817-836) in double, printed as std::cout prints a double."""
import math

import numpy as np

RULE = "------------------------------------------------\n"


def run_lengths(feat):
    """length of every maximal run of equal values: np.diff on the run heads"""
    feat = np.asarray(feat)
    if len(feat) == 0:
        return np.zeros(0, np.int64)
    heads = np.flatnonzero(np.concatenate([[True], feat[1:] != feat[:-1]]))
    return np.diff(np.concatenate([heads, [len(feat)]])).astype(np.int64)


def totals_of_lengths(length):
    ln = [int(x) for x in length]                   # Python integers: exact whatever the size
    hist = np.zeros(256, np.uint64)
    if ln:
        hist += np.bincount(np.minimum(np.asarray(ln, np.int64), 255), minlength=256).astype(np.uint64)
    return dict(n_buckets=len(ln), n_locations=sum(ln), sum2=sum(x * x for x in ln), sum3=sum(x * x * x for x in ln),
                max_size=max(ln) if ln else 0, hist=hist)


def totals(feat):
    return totals_of_lengths(run_lengths(feat))


def zero_totals():
    return totals_of_lengths([])


def add_totals(a, b):
    """the totals of two inputs together (two chunks, two shards)"""
    out = {k: a[k] + b[k] for k in ("n_buckets", "n_locations", "sum2", "sum3")}
    out["max_size"] = max(a["max_size"], b["max_size"])
    out["hist"] = a["hist"] + b["hist"]
    return out


def same_totals(a, b):
    return all(int(a[k]) == int(b[k]) for k in ("n_buckets", "n_locations", "sum2", "sum3", "max_size")) and np.array_equal(a["hist"], b["hist"])


def target_locations(tgt, n_targets):
    return np.bincount(np.asarray(tgt, np.int64), minlength=n_targets).astype(np.uint64)


def shard_features(shard):
    """one parsed shard file (oracle/dbfile.parse_shard) as the feature column of its triples"""
    return np.repeat(np.asarray(shard["keys"], np.uint32), np.diff(np.asarray(shard["off"]).astype(np.int64)))


# ----------------------------------------------------------------------------------------------------------------- the text
def reserve_buckets(n_keys):
    """hash_multimap::reserve_keys(n): size_type(1 + (1 / max_load_factor() * n)) with a float load factor of 0.8"""
    f = np.float32(1) / np.float32(0.8)
    f = np.float32(f * np.float32(n_keys))
    return int(np.float32(np.float32(1) + f))


def cout_double(x):
    """operator<<(double) with the stream's defaults: %g"""
    if math.isnan(x):
        return "-nan" if math.copysign(1.0, x) < 0 else "nan"
    return "%g" % x


def _div(a, b):
    """IEEE division (Python raises on a zero divisor)"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def moments(t):
    """(max, mean, stddev, skewness) of the bucket sizes as doubles, operation for operation as src/stat_moments.h has them"""
    n, s, s2sum, s3sum = float(t["n_buckets"]), float(t["n_locations"]), float(t["sum2"]), float(t["sum3"])
    size = int(t["n_buckets"])
    mean = s if size < 1 else _div(s, n)
    var = 0.0 if size < 1 else _div(s2sum - _div(s * s, n), n - 1)
    with np.errstate(all="ignore"):
        sd = float(np.sqrt(np.float64(var)))
    if size < 2:
        skew = 0.0
    else:
        n2, sq = n * n, s * s
        cm2 = _div(s2sum - _div(sq, n), n - 1)
        cm3 = _div(n2 * s3sum - 3 * n * (s * s2sum) + 2 * (sq * s), n * n2)
        try:
            p = math.pow(cm2, 1.5)
        except (ValueError, OverflowError):
            p = float("nan")
        skew = _div(cm3, p)
    return float(t["max_size"]), mean, sd, skew


def content_block(n_targets, n_ranked, n_tree_taxa, buckets, features, locations, t):
    """print_content_properties: the targets' lines, then -- with features -- the table's, then the closing rule"""
    out = ""
    if n_targets > 0:
        out += "targets              %d\nranked targets       %d\ntaxa in tree         %d\n" % (n_targets, n_ranked, n_tree_taxa)
    if features > 0:
        mx, mean, sd, skew = moments(t)
        out += RULE + "buckets              %d\n" % buckets
        out += "bucket size          max: %s mean: %s +/- %s <> %s\n" % tuple(cout_double(x) for x in (mx, mean, sd, skew))
        out += "features             %d\ndead features        0\nlocations            %d\n" % (features, locations)
    return out + RULE


def shard_block(shard, keep_first=0, remove_above=0):
    """the content block of one parsed shard file, under a bucket rule if one is given (tests/bucket_limit_ref.py)"""
    feat, tgt, win = shard_features(shard), shard["tgt"], shard["win"]
    n_keys = len(shard["keys"])
    if keep_first or remove_above:
        import bucket_limit_ref
        feat, tgt, win, _, _ = bucket_limit_ref.bucket_limit(feat, tgt, win, keep_first, remove_above)
    t = totals(feat)
    return content_block(*meta_counts(shard), reserve_buckets(n_keys), t["n_buckets"], t["n_locations"], t)


def meta_counts(shard):
    """(targets, ranked targets, taxa in tree) of a parsed shard file: a target is ranked when its taxon has a parent id other than
    0 (taxon::has_parent, src/taxonomy.h:308-310; taxon ids below zero are the targets', src/sketch_database.h:149-150)"""
    ranked = sum(1 for x in shard["taxa"] if x["id"] < 0 and x["parent"] != 0)
    return shard["target_count"], ranked, len(shard["taxa"]) - shard["target_count"]


def histogram_lines(t):
    return "".join("bucket size %d: %d\n" % (s, int(c)) for s, c in enumerate(t["hist"]) if c)


def locations_lines(names, windows, locs, sketch_size):
    """the `locations` mode: per target its name, windows, locations and locations / (windows x sketch size)"""
    out = "name\twindows\tlocations\tfill\n"
    for nm, w, l in zip(names, windows, locs):
        out += "%s\t%d\t%d\t%.3f\n" % (nm, int(w), int(l), (int(l) / (int(w) * sketch_size)) if int(w) else 0.0)
    return out


def parse_block(text):
    """the numbers of a recorded content block: dict(buckets, features, locations, max) -- what the whole-database check sums"""
    out = {}
    for line in text.split("\n"):
        for key in ("buckets", "features", "locations"):
            if line.startswith(key + " "):
                out[key] = int(line.split()[-1])
        if line.startswith("bucket size          max: "):
            out["max"] = int(float(line.split("max: ")[1].split()[0]))
    return out
