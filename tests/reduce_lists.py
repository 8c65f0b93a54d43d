"""Caller-made location lists for mcq_reduce (rows 8-11 alone), a plain second reference for them, and the routing rules
of the staged reduce restated so that a test can say which kernel a list met.

Nothing here comes from a genome or a fixture: the world is ~40 synthetic targets with 1, 2, 7, 64, 1000 and 70 000
windows, a tgt2tax in which some targets share a taxon, and a table of one key per target whose list holds the target's
first and last window -- so every location form of the handle knows every target's extent, and the bit-field form gets a
win_bits whose largest window id is in use.  The lists are the adversarial part: both sides of every length at which the
staged reduce changes kernel or register count, distinct-key counts on both sides of the limits of the de-duplicating
tail, ties, ranges exactly numWindows wide, empty virtual ranks, first and last windows, the last target, any order.

brute_reduce is written from the documented semantics, not from
the oracle's code; tests/test_reduce_lists.py holds the oracle to it on the whole corpus, which is what entitles the GPU
tests to trust the oracle on inputs no fixture contains."""
import numpy as np

U32 = np.uint64(0xFFFFFFFF)
TGT_STRIDE = 113                    # the window stride of the world's table: numWindows = 2 + max(query_len, insert_size_max) // 113
WIN_COUNTS = (1, 2, 7, 64, 1000, 70000)
N_TARGETS = 40
W_MAX = max(WIN_COUNTS)
LMAX = 16384                        # the GPU tests' workspaces: max_locs_per_query = 16384, so nothing is large
INSERT_HUGE = 1 << 33               # the m >= 2^31 branch of range_width

# routing constants of csrc/mcq_engine.hip, restated (a test that outlives a change of one of them fails in its coverage assertions)
LCAP_WAVE = 512                     # kLcapWave = MCQ_DEDUP_MAX_T
LCAP_WAVE16 = 1024                  # MCQ_LCAP_WAVE16
LCAP_BLOCK = 8192                   # kLcapBlock
DEDUP_MAX_D = 256                   # MCQ_DEDUP_MAX_D
OVF_CHUNK = 8                       # MCQ_OVF_CHUNK
FORCE_BLOCK_PATH, FORCE_RAW_SORT, NO_WAVE16, FOLD_BY_LISTS, QUIRK_SEQ_DROP = 0x100, 0x400, 0x800, 0x8000, 2

EDGE_T = [0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 383, 384, 385, 511, 512, 513,
          1023, 1024, 1025, 8064, 8065, 8191, 8192, 8193, LMAX - 1, LMAX]
SHORT_EDGE_T = [t for t in EDGE_T if t <= 513] + [1025, 8193]
EDGE_D = [1, 2, 63, 64, 65, 255, 256, 257]
NUM_WINDOWS = [2, 3, 8, 9, W_MAX - 1, W_MAX, W_MAX + 1]


def query_len_for(num_windows):
    """a query_len that gives this numWindows at insert_size_max = 0 (not the smallest one)"""
    return (num_windows - 2) * TGT_STRIDE + (50 if num_windows < 1000 else 0)


def num_windows_of(query_len, insert_size_max=0):
    return 2 + max(int(query_len), int(insert_size_max)) // TGT_STRIDE


class World:
    """tgt_windows u32[40], tgt2tax u32[40] and the tiny table (keys, off, locs) described above"""

    def __init__(self, seq_level=False):
        self.tgt_windows = np.array([WIN_COUNTS[t % len(WIN_COUNTS)] for t in range(N_TARGETS)], np.uint32)
        tax = np.zeros(N_TARGETS, np.uint32)
        for t in range(N_TARGETS):
            if t < 16:
                tax[t] = 1000 + t // 2          # neighbours share a taxon: different virtual ranks at every even P
            elif t < 28:
                tax[t] = 2000 + t % 4           # 16, 20, 24 (...) share one: the same virtual rank whenever P divides 4
            else:
                tax[t] = 3000 + t
            if seq_level and t % 5 == 3:
                tax[t] = 0x80000000 | t         # a target without an ancestor at the merge rank: what MCQ_QUIRK_SEQ_DROP drops
        self.tgt2tax = tax
        self.seq_level = seq_level
        locs, off = [], [0]
        for t in range(N_TARGETS):
            last = int(self.tgt_windows[t]) - 1
            locs += [(t << 32) | 0] + ([(t << 32) | last] if last else [])
            off.append(len(locs))
        self.keys = np.arange(1, N_TARGETS + 1, dtype=np.uint32) * np.uint32(2654435)
        self.off = np.array(off, np.uint64)
        self.locs = np.array(locs, np.uint64)

    def targets_with(self, n_windows):
        return [t for t in range(N_TARGETS) if self.tgt_windows[t] >= n_windows]


def loc(t, w):
    return (np.asarray(t, np.uint64) << np.uint64(32)) | np.asarray(w, np.uint64)


def to_native(locs64, db):
    """(tgt << 32) | win words in the word of the handle: bit fields (tgt << win_bits) | win, the global window index, or
    the 64-bit word itself.  The global-window offsets are the handle's own: from the tgt_windows it was given, else
    1 + the largest window id of each target in its table."""
    locs64 = np.ascontiguousarray(locs64, np.uint64)
    tgt, win = (locs64 >> np.uint64(32)).astype(np.int64), locs64 & U32
    if db.loc_bytes() == 8:
        return locs64.copy()
    import importlib
    eng = importlib.import_module("metacache-mpi_amd.engine")
    if db.layout()["loc_format"] == eng.MCQ_LOC_GLOBAL_WINDOW:
        keep = db._keep
        if len(keep) > 4:
            ext = keep[4].astype(np.int64)
        else:
            ext = np.zeros(len(keep[3]), np.int64)
            np.maximum.at(ext, (keep[2] >> np.uint64(32)).astype(np.int64), (keep[2] & U32).astype(np.int64) + 1)
        gw_off = np.concatenate([[0], np.cumsum(ext)]).astype(np.uint64)
        return (gw_off[tgt] + win).astype(np.uint32)
    return (((locs64 >> np.uint64(32)) << np.uint64(db.win_bits())) | win).astype(np.uint32)


# ------------------------------------------------------------------------------------------------ the plain reference
def _top_insert(top, cand, max_cand):
    """the bounded top list: an entry of a taxon already listed replaces it only with strictly more hits and then moves
    left past every entry with strictly fewer; a new taxon goes in front of the first entry with strictly fewer hits,
    if there is one or the list is not full; the list never grows beyond max_cand"""
    for i, e in enumerate(top):
        if e[0] == cand[0]:
            if cand[1] > e[1]:
                del top[i]
                while i > 0 and top[i - 1][1] < cand[1]:
                    i -= 1
                top.insert(i, cand)
            return
    j = 0
    while j < len(top) and top[j][1] >= cand[1]:
        j += 1
    if j < len(top) or len(top) < max_cand:
        top.insert(j, cand)
        del top[max_cand:]


def target_candidates(locs, num_windows):
    """one (target, hits, first window, last window) per target in ascending target order: for every start among the
    target's sorted windows the number of entries less than num_windows windows to its right; the first strictly
    largest count"""
    locs = np.asarray(locs, np.uint64)
    tgt, win = (locs >> np.uint64(32)).astype(np.int64), (locs & U32).astype(np.int64)
    out = []
    for t in np.unique(tgt).tolist():
        w = np.sort(win[tgt == t])
        cnt = np.searchsorted(w, w + int(num_windows), side="left") - np.arange(len(w))
        b = int(np.argmax(cnt))                     # (numpy: the first of equal maxima)
        out.append((t, int(cnt[b]), int(w[b]), int(w[b + int(cnt[b]) - 1])))
    return out


def brute_reduce(locs, num_windows, tgt2tax, max_cand, _cands=None):
    """rows 8-11 at P = 1: (uint32 [n, 4] of (taxon, hits, first window, last window), n)"""
    top = []
    for t, hits, beg, end in (target_candidates(locs, num_windows) if _cands is None else _cands):
        _top_insert(top, (int(tgt2tax[t]), hits, beg, end), max_cand)
    return np.array(top, np.uint32).reshape(-1, 4), len(top)


# ------------------------------------------------------------------------------------------------ routing, restated
def pow2ceil(n):
    p = 1
    while p < n:
        p *= 2
    return p


def list_form(P, M, flags, seq_taxa):
    """how the P top lists are kept (make_opt): 'p1'; 'lin' = rows 10-11 as one selection; 'lanes' = P lists side by side
    in a wave's 64 lanes; 'big' = P lists in the workgroup kernel's LDS, which then takes every query"""
    if P == 1:
        return "p1"
    if not (flags & FOLD_BY_LISTS) and not ((flags & QUIRK_SEQ_DROP) and seq_taxa):
        return "lin"
    return "big" if pow2ceil(P) * M > 64 else "lanes"


def route(T, D, num_windows, loc_bytes, flags, form, lmax=LMAX):
    """the kernel and the branch of it that a list of T words with D distinct ones meets in mcq_reduce"""
    block_only = bool(flags & FORCE_BLOCK_PATH) or form == "big"
    if T > LCAP_WAVE or block_only:
        if loc_bytes == 4 and LCAP_WAVE < T <= LCAP_WAVE16 and not block_only and not (flags & NO_WAVE16):
            return "wave16"
        if T > lmax:
            return "capacity"
        if T == 0:
            return "block-empty"
        if ((T + 127) & ~127) <= LCAP_BLOCK and pow2ceil(T) <= 8192:
            return "block-lds"
        return "block-global"
    if T == 0:
        return "wave-empty"
    if loc_bytes == 8:
        return "wave64"
    if (flags & FORCE_RAW_SORT) or D > DEDUP_MAX_D:
        return "wave-raw"
    return "wave-dedup-regs" if D <= 64 and num_windows <= 8 else "wave-dedup-weighted"


def queue_of(cls):
    return {"wave16": "mid", "capacity": "block", "block-empty": "block", "block-lds": "block", "block-global": "block"}.get(cls, "none")


# ------------------------------------------------------------------------------------------------ the corpus
class _Gen:
    def __init__(self, world, seed):
        self.w = world
        self.tw = world.tgt_windows.astype(np.int64)
        self.rng = np.random.default_rng(seed)
        self.groups = []
        self.n = 0

    def order(self, a):
        """(h) any order inside: two lists of three shuffled, one sorted, and now and then one sorted downwards"""
        a = np.ascontiguousarray(a, np.uint64)
        self.n += 1
        if self.n % 3 == 0:
            return np.sort(a)
        if self.n % 7 == 0:
            return np.sort(a)[::-1].copy()
        return self.rng.permutation(a)

    def add(self, lists, nw, what):
        lists = [self.order(x) for x in lists]
        for x in lists:         # inside the world: the global-window form has no word for anything else
            assert ((x >> np.uint64(32)) < N_TARGETS).all() and ((x & U32).astype(np.int64) < self.tw[(x >> np.uint64(32)).astype(np.int64)]).all(), what
        self.groups.append((lists, query_len_for(nw), what))

    def universe(self, targets, span):
        parts = []
        for t in targets:
            n = int(min(span, self.tw[t]))
            base = int(self.rng.integers(0, self.tw[t] - n + 1))
            parts.append(loc(t, base + np.arange(n)))
        return np.concatenate(parts)

    def multiset(self, T, D, targets, span, exact=True):
        """T words with exactly D distinct ones (exact=False: at most D), inside a few windows of a few targets so that
        ranges compete"""
        if T == 0:
            return np.zeros(0, np.uint64)
        u = self.universe(targets, span)
        assert len(u) >= D or not exact, (len(u), D)
        D = min(D, len(u))
        base = self.rng.choice(u, size=D, replace=False)
        return np.concatenate([base, self.rng.choice(base, size=T - D)])


def corpus(world, lmax=LMAX):
    """list of (lists, query_len, what); every list a uint64 array of (tgt << 32) | win, in any order"""
    g = _Gen(world, 20240)
    rng, tw = g.rng, g.tw
    wide = world.targets_with(W_MAX)                # 70 000 windows
    mid = world.targets_with(1000)
    edge_t = [t for t in EDGE_T if t <= lmax]
    for nw in NUM_WINDOWS:
        Ts = edge_t if nw in (3, 9) else SHORT_EDGE_T
        # (a) one (target, window) T times
        ts = rng.integers(0, N_TARGETS, size=len(Ts))
        g.add([np.full(T, loc(t, rng.integers(0, tw[t]))) for T, t in zip(Ts, ts)], nw, "a:repeat nw=%d" % nw)
        # (b) one target, consecutive windows once each
        g.add([loc(wide[i % len(wide)], int(rng.integers(0, W_MAX - T + 1)) + np.arange(T)) for i, T in enumerate(Ts)], nw,
              "b:consecutive nw=%d" % nw)
        # every length again with a few targets, a few windows each, many copies
        g.add([g.multiset(T, min(T, [1, 40, 64, 200, 256, 700][i % 6]), list(rng.choice(mid, size=3, replace=False)) + [int(rng.integers(0, N_TARGETS))],
                          max(3 * min(nw, 80), 240)) for i, T in enumerate(Ts)], nw, "T-edges nw=%d" % nw)
        # distinct keys on both sides of 64 and 256, T up to the first stage's 512
        dl = []
        for D in EDGE_D:
            for T in sorted({D, D + 1, min(512, 2 * D), 511 if D > 64 else 65, 512}):
                dl.append(g.multiset(T, D, list(rng.choice(mid, size=4, replace=False)), max(4, 3 * min(nw, 40), D // 3 + 1)))
        g.add(dl, nw, "D-edges nw=%d" % nw)
        # (c) two ranges of one target with the same count, at least numWindows apart: the first wins; with one more hit in the
        # second, the second does
        cl = []
        for c in (1, 2, 32, 128, 256, 300, 600, 4097):
            k = min(c, nw, 50)                       # distinct windows of a range
            fits = [t for t in range(N_TARGETS) if tw[t] >= 2 * k + nw + 3]
            if not fits:
                continue
            for more in (0, 1):
                t = int(rng.choice(fits))
                w0 = int(rng.integers(0, tw[t] - (2 * k + nw + 2)))
                gap = int(rng.integers(0, 3))
                first = loc(t, w0 + np.arange(c) % k)
                second = loc(t, w0 + k - 1 + nw + gap + np.arange(c + more) % k)
                other = int(rng.integers(0, N_TARGETS))
                cl.append(np.concatenate([first, second, np.full(c if other != t else 0, loc(other, 0))]))      # and a tie with another target
        g.add(cl, nw, "c:two-ranges nw=%d" % nw)
        # (d) hits at w and w + numWindows - 1 are one range; with the second at w + numWindows they are two
        dl = []
        for m1, m2 in ((1, 1), (1, 2), (2, 1), (100, 100), (255, 257), (300, 300), (520, 520)):
            for apart in (0, 1):
                fits = [t for t in range(N_TARGETS) if tw[t] >= nw + apart]
                if not fits:
                    continue
                t = int(rng.choice(fits))
                w = int(rng.choice([0, tw[t] - nw - apart, int(rng.integers(0, tw[t] - nw - apart + 1))]))     # first window, last window, anywhere
                dl.append(np.concatenate([np.full(m1, loc(t, w)), np.full(m2, loc(t, w + nw - 1 + apart))]))
        g.add(dl, nw, "d:range-width nw=%d" % nw)
    for nw in (3, 9):
        # (e) k targets with the same count (more than max_cand x P of them for the small P and max_cand), and one a hit ahead
        el = []
        for k, c in ((3, 1), (5, 2), (9, 1), (17, 12), (33, 3), (40, 1), (40, 12), (40, 30), (40, 210)):
            for ahead in (0, 1):
                ts = rng.permutation(N_TARGETS)[:k]
                parts = [loc(t, int(rng.integers(0, tw[t])) + np.zeros(c, np.int64)) for t in ts]
                if ahead:
                    parts.append(parts[int(rng.integers(0, k))][:1])
                el.append(np.concatenate(parts))
        g.add(el, nw, "e:ties nw=%d" % nw)
        # (f) all targets congruent mod m: one virtual rank holds everything; and a few targets that leave ranks empty
        fl = []
        for m in (2, 3, 8, 32):
            for T in (40, 300, 700, 1500):
                r = int(rng.integers(0, m))
                ts = list(range(r, N_TARGETS, m))
                fl.append(g.multiset(T, min(T, 60), ts, 40, exact=False))
        for ts in ([0, 1, 5], [39], [4, 36], [7, 10, 11, 35]):
            for T in (12, 600, 1100):
                fl.append(g.multiset(T, min(T, 30), ts, 12, exact=False))
        g.add(fl, nw, "f:ranks nw=%d" % nw)
        # (g) windows 0 and last, and the last target
        gl = []
        for t in (0, 1, 2, 3, 4, 5, 35, N_TARGETS - 1):
            a, b = int(rng.integers(1, 5)), int(rng.integers(1, 5))
            gl.append(np.concatenate([np.full(a, loc(t, 0)), np.full(b, loc(t, tw[t] - 1))]))
        every = np.concatenate([loc(np.arange(N_TARGETS), 0), loc(np.arange(N_TARGETS), tw - 1)])
        gl += [every, np.repeat(every, 7), np.repeat(every, 14), np.repeat(every, 110)]
        g.add(gl, nw, "g:extremes nw=%d" % nw)
    return g.groups


def flatten(groups):
    """(lists, query_len uint32 per list, what per list)"""
    lists, qlen, what = [], [], []
    for ls, q, w in groups:
        lists += ls
        qlen += [q] * len(ls)
        what += [w] * len(ls)
    return lists, np.array(qlen, np.uint32), what


def counter_wrap_lists(world):
    """(i) 66 000 copies of one location -- more than a 16-bit counter holds -- alone, beside a second target, and split
    over two windows of one range; for a workspace of its own with lmax = 2^17"""
    t = world.targets_with(1000)[0]                 # 1000 windows
    other = world.targets_with(W_MAX)[1]            # of another taxon
    assert world.tgt2tax[t] != world.tgt2tax[other]
    one = np.full(66000, loc(t, 999))
    return [one, np.concatenate([np.full(3, loc(0, 0)), one, np.full(30000, loc(other, 5))]),
            np.concatenate([np.full(33000, loc(t, 10)), np.full(33000, loc(t, 11)), np.full(100, loc(t, 500))])]
