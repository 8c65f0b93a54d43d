"""TEST CODE: plain NumPy references of what the staged entry points of csrc/mcq_stages.hip compute, one stage each
(no GPU, no native code).  tests/test_stage_refs.py ties them to the oracle on the CPU; tests/test_gpu_stage_edges.py
compares the kernels with them.

All integer arithmetic is written out in uint64 so that nothing depends on NumPy's promotion rules.
"""
import numpy as np

EMPTY = 0xFFFFFFFF
_M32 = np.uint64(0xFFFFFFFF)
_U = np.uint64


# ------------------------------------------------------------------ row 1: windows (for_each_window)
def num_windows(n, W, S):
    """windows of sequences of n bases (array or scalar) -> uint64 array.  A sequence of at most W bases (an empty one
    included) is one window; a longer one has nfull = (n - W) // S + 1 full windows and one more, shorter, if
    nfull * S < n."""
    n = np.atleast_1d(np.asarray(n, dtype=np.uint64))
    W, S = _U(W), _U(S)
    long_ = n > W
    nfull = np.where(long_, (np.where(long_, n, W) - W) // S + _U(1), _U(1))
    return np.where(long_, nfull + (nfull * S < n).astype(np.uint64), _U(1))


def windows(n, W, S):
    """[(begin, end)] of the windows of a sequence of n bases"""
    n, W, S = int(n), int(W), int(S)
    if n <= W:
        return [(0, n)]
    nfull = (n - W) // S + 1
    out = [(j * S, j * S + W) for j in range(nfull)]
    if nfull * S < n:
        out.append((nfull * S, n))
    return out


# ------------------------------------------------------------------ routing: owner of a feature
def tmh(x):
    """Thomas Mueller's 32-bit hash of uint32 values (array) -> uint64 array below 2^32"""
    x = np.atleast_1d(np.asarray(x)).astype(np.uint64) & _M32
    c = _U(0x45D9F3B)
    x = (((x >> _U(16)) ^ x) * c) & _M32
    x = (((x >> _U(16)) ^ x) * c) & _M32
    return (x >> _U(16)) ^ x


def owner(f, n_shards):
    """owning shard of every feature: (tmh(f) * n_shards) >> 32; -1 for the dropped value 0xFFFFFFFF.  int64 array"""
    f = np.atleast_1d(np.asarray(f)).astype(np.uint64) & _M32
    own = ((tmh(f) * _U(n_shards)) >> _U(32)).astype(np.int64)
    own[f == _U(EMPTY)] = -1
    return own


# ------------------------------------------------------------------ scan
def exclusive_scan(x):
    """uint64 [n + 1]: out[i] = sum of x[:i]; out[n] is the total"""
    x = np.asarray(x).astype(np.uint64).ravel()
    out = np.zeros(len(x) + 1, np.uint64)
    np.cumsum(x, out=out[1:])
    return out


# ------------------------------------------------------------------ mcq_bucket_features
def bucket(features, n_shards):
    """-> (counts uint64 [n_shards], [ascending source indices of shard 0, of shard 1, ...])"""
    own = owner(features, n_shards)
    key = np.where(own < 0, 255, own).astype(np.uint8)                  # n_shards <= 64
    order = np.argsort(key, kind="stable")
    counts = np.bincount(key, minlength=256)[:n_shards].astype(np.uint64)
    cut = np.cumsum(counts.astype(np.int64))
    return counts, np.split(order[:int(cut[-1]) if n_shards else 0].astype(np.int64), cut[:-1])


# ------------------------------------------------------------------ mcq_assemble
def assemble(list_len, src_slot, n_slots, src_locs, seq_len, win_off, s, paired):
    """List i (list_len[i] words, one list after the other in src_locs) belongs to feature slot src_slot[i] of the
    batch's [window][s] feature array; the output holds the lists in slot order.
    -> (dst_locs [total], loc_off uint64 [nq + 1], query_len uint32 [nq]): query q's segment starts at the first slot of
    its first window (window win_off[q], or win_off[2q] when paired) and its length is that of its mates together."""
    list_len = np.asarray(list_len).astype(np.uint64).ravel()
    src_slot = np.asarray(src_slot).astype(np.int64).ravel()
    src_locs = np.asarray(src_locs).ravel()
    seq_len = np.asarray(seq_len).astype(np.uint64).ravel()
    win_off = np.asarray(win_off).astype(np.uint64).ravel()
    slot_len = np.zeros(n_slots, np.uint64)
    slot_len[src_slot] = list_len
    dst_off = exclusive_scan(slot_len)
    src_off = exclusive_scan(list_len)
    total = int(src_off[-1])
    assert total == int(dst_off[-1]), "a slot is named by two lists"
    dst = np.zeros(total, src_locs.dtype)
    shift = dst_off[src_slot].astype(np.int64) - src_off[:-1].astype(np.int64)
    dst[np.arange(total, dtype=np.int64) + np.repeat(shift, list_len.astype(np.int64))] = src_locs[:total]
    step = 2 if paired else 1
    nq = len(seq_len) // step
    first = np.arange(nq, dtype=np.int64) * step
    loc_off = np.empty(nq + 1, np.uint64)
    loc_off[:nq] = dst_off[(win_off[first] * _U(s)).astype(np.int64)]
    loc_off[nq] = dst_off[n_slots]
    qlen = seq_len[first].copy()
    if paired:
        qlen += seq_len[first + 1]
    return dst, loc_off, (qlen & _M32).astype(np.uint32)


# ------------------------------------------------------------------ location words
def decode_native(db, words, gw_off=None):
    """location words in a handle's native form -> (tgt << 32) | win as uint64.  db: engine.Database; gw_off: for the
    global-window form, the first window of every target (prefix sums of the windows per target, [n_targets + 1])."""
    w = np.asarray(words)
    if db.loc_bytes() == 8:                                             # (tgt << 32) | win
        return w.view(np.uint64).copy() if w.dtype.itemsize == 8 else w.astype(np.uint64)
    w = (w.view(np.uint32) if w.dtype.itemsize == 4 else w).astype(np.uint64)
    if db.layout()["loc_format"] == 2:                                  # MCQ_LOC_GLOBAL_WINDOW: gw_off[tgt] + win
        g = np.asarray(gw_off).astype(np.uint64)
        t = np.searchsorted(g, w, side="right").astype(np.int64) - 1
        return (t.astype(np.uint64) << _U(32)) | (w - g[t])
    wb = _U(db.win_bits())                                              # (tgt << win_bits) | win
    return ((w >> wb) << _U(32)) | (w & ((_U(1) << wb) - _U(1)))
