"""What the -remove-ambig-features tests share (tests/test_gpu_ambig.py, tests/test_gpu_build_cli_ambig.py): the NumPy statement of
remove_ambiguous_features (src/sketch_database.h:428-470) on a table -- distinct (key index, tgt_key[target]) pairs per key -- the
same kind of reference as _numpy_split of tests/test_gpu_build_cli.py."""
import numpy as np


def ambiguous_keys(off, locs, tgt_key, max_keys):
    """bool per key: its list names more than max_keys distinct tgt_key[target]"""
    n_keys = len(off) - 1
    key_of = np.repeat(np.arange(n_keys, dtype=np.int64), np.diff(off.astype(np.int64)))
    clade = np.asarray(tgt_key, np.uint32)[(locs >> np.uint64(32)).astype(np.int64)].astype(np.int64)
    pairs = np.unique(key_of * (1 << 32) + clade)                 # distinct (key index, clade) pairs
    return np.bincount(pairs >> 32, minlength=n_keys) > max_keys


def numpy_filter(keys, off, locs, tgt_key, max_keys):
    """(keys, list_off, locs, n_removed) of the table without its ambiguous keys: lists unchanged, order kept"""
    drop = ambiguous_keys(off, locs, tgt_key, max_keys)
    lens = np.diff(off.astype(np.int64))
    o = np.zeros(int((~drop).sum()) + 1, np.uint64)
    o[1:] = np.cumsum(lens[~drop])
    return keys[~drop], o, locs[np.repeat(~drop, lens)], int(drop.sum())


def filter_triples(tri, tgt_key, max_keys):
    """the same on (feature, target, window) rows (any order, all ranks of a database together): the rows of the features that stay"""
    feat = tri[:, 0].astype(np.uint64)
    clade = np.asarray(tgt_key, np.uint32)[tri[:, 1].astype(np.int64)].astype(np.uint64)
    pairs = np.unique((feat << np.uint64(32)) | clade)            # distinct (feature, clade) pairs
    f, n = np.unique(pairs >> np.uint64(32), return_counts=True)
    bad = f[n > max_keys]
    return tri[~np.isin(feat, bad)], len(bad), len(f)
