"""A NumPy statement of the query-time bucket rules: what mcq_bucket_limit does to a chunk of
(feature, target, window) triples, and how the reference's two options become the rule (include/mcq_open.hpp, mcq_bucket_rule).

The chunk rule: a maximal run of equal `feat` is one bucket of one rank (the chunk holds whole key records of one shard
file).  Removal first (remove_features_with_more_locations_than, src/sketch_database.h:381-395), then the shrink
(max_locations_per_feature, src/sketch_database.h:356-368)."""
import numpy as np

MAX_SUPPORTED = 254          # database::max_supported_locations_per_feature(): the 8-bit bucket size type's maximum - 1


def runs(feat):
    """(start, length) of every maximal run of equal values"""
    feat = np.asarray(feat)
    if len(feat) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    start = np.flatnonzero(np.concatenate([[True], feat[1:] != feat[:-1]])).astype(np.int64)
    return start, np.diff(np.concatenate([start, [len(feat)]]))


def bucket_limit(feat, tgt, win, keep_first=0, remove_above=0):
    """-> (feat, tgt, win, n_shrunk, n_removed): the triples that stay, in their order, and the buckets shrunk / removed"""
    feat, tgt, win = (np.asarray(x, np.uint32) for x in (feat, tgt, win))
    start, length = runs(feat)
    if len(feat) == 0 or (not keep_first and not remove_above):
        return feat.copy(), tgt.copy(), win.copy(), 0, 0
    removed = (length > remove_above) if remove_above else np.zeros(len(length), bool)
    shrunk = ~removed & (length > keep_first) if keep_first else np.zeros(len(length), bool)
    run_of = np.repeat(np.arange(len(start)), length)
    pos = np.arange(len(feat)) - start[run_of]
    keep = ~removed[run_of] & ~(shrunk[run_of] & (pos >= keep_first))
    return feat[keep], tgt[keep], win[keep], int(shrunk.sum()), int(removed.sum())


def bucket_rule(max_locs, remove_overpopulated, db_limit):
    """(-max-locations-per-feature N, -remove-overpopulated-features, the database's own limit) -> (keep_first, remove_above),
    0 = that rule is off.  src/mode_query.cpp:354-377, line for line."""
    keep_first = remove_above = 0

    def setter(n):                                  # max_locations_per_feature(bucket_size_type n), src/sketch_database.h:356-368
        n &= 0xFF                                   # the argument has the 8-bit bucket size type
        if n < 1:
            n = 1
        if n >= MAX_SUPPORTED:                      # "the largest": the limit is set, nothing is shrunk
            return 0
        return n if n < db_limit else 0             # shrinks only below the database's limit

    if remove_overpopulated:
        maxlpf = max_locs - 1
        if maxlpf < 0 or maxlpf >= MAX_SUPPORTED:
            maxlpf = MAX_SUPPORTED - 1
        maxlpf = min(maxlpf, db_limit - 1)
        if maxlpf > 0:                              # "always keep buckets with size 1"
            remove_above = maxlpf
        keep_first = setter(max_locs)
    elif max_locs > 1:
        keep_first = setter(max_locs)
    return keep_first, remove_above


def filter_shard(shard, keep_first, remove_above):
    """the rule on one parsed shard file (oracle/dbfile.py): every key is one bucket of that rank.  -> a dict with the keys
    that keep a location, off, tgt, win, as dbfile.union_shards takes it"""
    length = np.diff(np.asarray(shard["off"]).astype(np.int64))
    feat = np.repeat(np.asarray(shard["keys"], np.uint32), length)
    f, t, w, _, _ = bucket_limit(feat, shard["tgt"], shard["win"], keep_first, remove_above)
    start, ln = runs(f)
    return dict(keys=f[start], off=np.concatenate([[0], np.cumsum(ln)]).astype(np.uint64), tgt=t, win=w)
