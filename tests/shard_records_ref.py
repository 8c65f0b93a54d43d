"""The key records of a shard file in numpy: what mcq_refdb_write_shard writes behind its two counts for a table, and what
mcq_table_shard_records makes on the GPU.  Per key with a non-empty list, in key order:
`u32 key, u8 n, u64 n, u32 tgt[n], u64 n, u32 win[n]` -- 21 + 8 n bytes, little-endian, no padding."""
import numpy as np


def serialize(keys, list_off, locs):
    """(keys u32 [n], list_off u64 [n + 1], locs u64 (tgt << 32 | win)) -> numpy uint8 array of the records"""
    keys = np.asarray(keys, np.uint32)
    off = np.asarray(list_off, np.uint64).astype(np.int64)
    locs = np.asarray(locs, np.uint64)
    n = np.diff(off)
    assert (n >= 0).all() and (n <= 255).all()
    live = n > 0
    keys, n, beg = keys[live], n[live], off[:-1][live]
    size = 21 + 8 * n
    at = np.zeros(len(n) + 1, np.int64)
    at[1:] = np.cumsum(size)
    out = np.zeros(int(at[-1]), np.uint8)

    def put(pos, values, width):
        """little-endian `values` of `width` bytes at the byte positions `pos`"""
        v = np.asarray(values, np.uint64)
        for b in range(width):
            out[pos + b] = ((v >> np.uint64(8 * b)) & np.uint64(0xFF)).astype(np.uint8)

    at0 = at[:-1]
    put(at0, keys, 4)
    put(at0 + 4, n, 1)
    put(at0 + 5, n, 8)
    put(at0 + 13 + 4 * n, n, 8)
    # every location: its record, its index inside the list
    rec = np.repeat(np.arange(len(n), dtype=np.int64), n)
    j = np.arange(int(n.sum()), dtype=np.int64) - np.repeat(np.cumsum(n) - n, n)
    src = np.repeat(beg, n) + j
    put(at0[rec] + 13 + 4 * j, locs[src] >> np.uint64(32), 4)
    put(at0[rec] + 21 + 4 * n[rec] + 4 * j, locs[src] & np.uint64(0xFFFFFFFF), 4)
    return out, int(live.sum()), int(n.sum())
