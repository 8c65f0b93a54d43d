"""Every staged entry point of csrc/mcq_stages.hip alone, against the plain references of tests/stage_refs.py (which
tests/test_stage_refs.py ties to the oracle), at the sizes where its kernels change shape: mcq_count_windows and the
exclusive scan under it, both kernels of mcq_sketch, mcq_bucket_features, mcq_assemble, and mcq_lookup_count / _gather
with kept list starts.  All comparisons are exact.  Every output buffer is a little larger than needed and prefilled
with a sentinel: what lies behind the output must come back untouched.  Each test asserts what it covered."""
import functools
import importlib

import numpy as np
import pytest
import torch

import stage_refs as ref
from oracle import mc_oracle as orc

pytestmark = pytest.mark.gpu

# (k, s, W, S)
GEOMETRIES = [(16, 16, 128, 113), (12, 8, 64, 53), (16, 16, 128, 64), (8, 4, 100, 93), (1, 3, 20, 20), (16, 16, 128, 1)]
SCAN_TILE = 8192                    # MCQ_SCAN_TILE: one workgroup up to here, three launches beyond
SENT = 0x5A5A5A5A
TAIL = 7
EMPTY = 0xFFFFFFFF


@pytest.fixture(scope="module")
def eng():
    return importlib.import_module("metacache-mpi_amd.engine")


def _dev():
    return torch.device("cuda", 0)


def _empty_db(eng, geom, flags=0):
    k, s, W, S = geom
    return eng.Database(np.zeros(0, np.uint32), np.zeros(1, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint32),
                        k=k, sketch_size=s, winlen=W, winstride=S, flags=flags)


def _up(a, dtype):
    """numpy unsigned array -> device tensor of the signed type of the same width (never empty)"""
    a = np.ascontiguousarray(a).view({torch.int32: np.int32, torch.int64: np.int64, torch.uint8: np.uint8}[dtype])
    return torch.from_numpy(a.copy()).to(_dev()) if a.size else torch.zeros(1, dtype=dtype, device=_dev())


def _out(n, dtype):
    """output buffer of n elements plus a tail, all sentinel"""
    fill = SENT if dtype == torch.int32 else (SENT << 32) | SENT
    return torch.full((n + TAIL,), fill, dtype=dtype, device=_dev())


def _down(t, n, what):
    """the first n elements as an unsigned numpy array, after checking that the tail was left alone"""
    fill = SENT if t.dtype == torch.int32 else (SENT << 32) | SENT
    assert bool((t[n:] == fill).all()), "%s: written behind the output" % what
    return t[:n].cpu().numpy().view(np.uint32 if t.dtype == torch.int32 else np.uint64)


def _layout(seq_len, ranges, rng):
    """seq_off of sequences of these lengths (uint64): offsets, or [begin, end) pairs whose sequences lie in a shuffled
    order, so the pairs are not ascending"""
    seq_len = np.asarray(seq_len, np.uint64)
    if not ranges:
        return ref.exclusive_scan(seq_len)
    perm = rng.permutation(len(seq_len))
    beg = np.zeros(len(seq_len), np.uint64)
    beg[perm] = ref.exclusive_scan(seq_len[perm])[:-1]
    return np.stack([beg, beg + seq_len], axis=1).ravel()


# ====================================================================================== a. mcq_count_windows + scan
CW_NSEQS = [0, 1, 63, 64, 65, 255, 256, 257, 8191, 8192, 8193, 16384, 16385, 8192 * 256, 8192 * 256 + 1, 8192 * 257 + 77]
CW_CASES = [(n, i % len(GEOMETRIES), False) for i, n in enumerate(CW_NSEQS)] + [(8193, 0, True)]


def _cw_length_set(geom):
    k, _, W, S = geom
    vals = {0, 1, k - 1, k, W - 1, W, W + 1, W + S - 1, W + S, W + S + 1, 1 << 33}
    for n in range(W + 1, W + 5 * S + 1):          # the last full window ends the sequence: no short window behind it
        nfull = (n - W) // S + 1
        if nfull * S == n and nfull <= 5:
            vals.add(n)
    return np.array(sorted(vals), np.uint64)


@pytest.mark.parametrize("n,gi,ranges", CW_CASES, ids=["%d-g%d%s" % (n, gi, "-ranges" if r else "") for n, gi, r in CW_CASES])
def test_count_windows_and_scan_edges(eng, n, gi, ranges):
    """win_off = exclusive scan of the window counts, at every size where the scan changes shape: one workgroup up to 8192
    elements, three launches beyond, and a tile-sum scan that loops with a carry from 257 tiles on (256 threads)"""
    assert sorted({c[0] for c in CW_CASES}) == CW_NSEQS and any(c[2] for c in CW_CASES) and not all(c[2] for c in CW_CASES)
    assert {c[1] for c in CW_CASES} == set(range(len(GEOMETRIES)))
    tiles = [(m + SCAN_TILE - 1) // SCAN_TILE for m in CW_NSEQS]
    assert sum(t > 256 for t in tiles) == 2 and any(m // SCAN_TILE > 256 for m in CW_NSEQS)      # the carry loop runs
    assert {m for m in CW_NSEQS if m % SCAN_TILE == 0 and m} == {8192, 16384, 8192 * 256}         # n on a tile edge
    geom = GEOMETRIES[gi]
    _, _, W, S = geom
    rng = np.random.default_rng(1000 + n)
    vals = _cw_length_set(geom)
    lens = rng.choice(vals, size=n)
    if n >= len(vals):
        lens[:len(vals)] = vals                     # every length at least once ...
        rng.shuffle(lens)
        assert (lens == np.uint64(1 << 33)).any()
    if ranges:                                      # ... and pairs that overlap, out of order
        beg = rng.integers(0, 1 << 20, size=n).astype(np.uint64)
        seq_off = np.stack([beg, beg + lens], axis=1).ravel()
        assert (np.diff(beg.astype(np.int64)) < 0).any()
    else:
        seq_off = ref.exclusive_scan(lens)
    want = ref.exclusive_scan(ref.num_windows(lens, W, S)) if n else np.zeros(1, np.uint64)
    db = _empty_db(eng, geom)
    bases = torch.zeros(1, dtype=torch.uint8, device=_dev())            # the kernel reads seq_off only
    so = _up(seq_off, torch.int64)
    win_off = _out(n + 1, torch.int64)
    db.count_windows(bases.data_ptr(), so.data_ptr(), n, win_off.data_ptr(), flags=eng.MCQ_BATCH_RANGES if ranges else 0)
    torch.cuda.synchronize()
    got = _down(win_off, n + 1, "win_off")
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (geom, n, "first difference at", bad[:3], got[bad[:3]], want[bad[:3]])


# ====================================================================================== b. mcq_sketch, both kernels
SK_BATCHES = [300, 4095, 4096, 12000]
SK_PADS = [0, 1, 3]
SK_SEQS_KERNEL_FROM = 4096          # mcq_sketch: one wave per sequence from here on, one wave per window below
IUPAC = np.frombuffer(b"NRYKMSWBDHVn-", np.uint8)


def _sk_make(rng, L, variant, k, W):
    a = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=L)
    if variant == 1 and L:
        a[rng.integers(0, L, size=max(1, L // 50))] = rng.choice(IUPAC, size=max(1, L // 50))
        first = min(L, W)
        a[first - 1 - int(rng.integers(0, min(k, first)))] = ord("N")           # inside the last k-mer of the first window
        a[L - 1 - int(rng.integers(0, min(k, L)))] = ord("N")                   # ... and of the sequence
    if variant == 2:
        a[:L // 2] |= 0x20
    return a.tobytes()


@functools.lru_cache(maxsize=None)
def _sk_set(geom):
    """300 sequences of one geometry with the expected rows of each, computed once: (seqs, rows [n_win, s] per sequence,
    n_feat per sequence, order of the 12 000 batch)"""
    k, s, W, S = geom
    rng = np.random.default_rng(77 + 1000 * GEOMETRIES.index(geom))
    nw = lambda n: int(ref.num_windows(n, W, S)[0])
    lengths = set(range(0, k + 2))
    for n in range(1, W + 6 * S + 3):
        if nw(n) != nw(n - 1) and nw(n) <= 6:       # the window count changes at n
            lengths |= {max(0, n - 2), n - 1, n, n + 1}
    seqs = [_sk_make(rng, L, v, k, W) for L in sorted(lengths) for _ in range(2) for v in range(3)]
    seqs += [_sk_make(rng, L, v, k, W) for L in (500, 1017, 4000, 20000) for v in range(3)]
    assert 100 <= len(seqs) <= 300, len(seqs)
    while len(seqs) < 300:
        seqs.append(_sk_make(rng, int(rng.integers(0, 3 * W)), int(rng.integers(0, 3)), k, W))
    rows, nfeat = [], []
    for sq in seqs:
        wins = ref.windows(len(sq), W, S)
        r = np.full((len(wins), s), EMPTY, np.uint32)
        m = np.zeros(len(wins), np.uint32)
        for j, (b, e) in enumerate(wins):
            f = orc.sketch(sq[b:e], k, s)
            r[j, :len(f)] = f
            m[j] = len(f)
        rows.append(r); nfeat.append(m)
    order = np.concatenate([np.arange(300)] + [rng.permutation(300) for _ in range(39)])
    assert len(order) == 12000
    return seqs, rows, nfeat, order


def _first_row_diff(got, want, s):
    w = int(torch.nonzero((got.view(-1, s) != want.view(-1, s)).any(dim=1))[0])
    return w, got.view(-1, s)[w].cpu().numpy().view(np.uint32), want.view(-1, s)[w].cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("geom", GEOMETRIES, ids=["-".join(map(str, g)) for g in GEOMETRIES])
def test_sketch_both_kernels_every_geometry(eng, geom):
    """one wave per window (below 4096 sequences: 64-bit window arithmetic, binary search in win_off) and one wave per
    sequence (from 4096 on: 32-bit arithmetic, division by the stride as a multiplication) give the oracle's sketch of
    every window, for every geometry, base-pointer alignment and batch form -- and the same bytes as each other"""
    k, s, W, S = geom
    seqs, rows, nfeat, order = _sk_set(geom)
    assert any(len(m) > 1 for m in nfeat) and any((m == 0).any() for m in nfeat) and any((m > 0).all() for m in nfeat)
    assert min(SK_BATCHES) < SK_SEQS_KERNEL_FROM <= max(SK_BATCHES) and {4095, 4096} <= set(SK_BATCHES)
    db = _empty_db(eng, geom)
    rng = np.random.default_rng(5)
    lens = np.array([len(x) for x in seqs], np.uint64)
    # ranges form: the 300 sequences once, in a shuffled order; a batch's pairs point into that text
    text_r_off = _layout(lens, True, rng).reshape(-1, 2)
    text_r = np.zeros(int(lens.sum()), np.uint8)
    for i, sq in enumerate(seqs):
        text_r[int(text_r_off[i, 0]):int(text_r_off[i, 1])] = np.frombuffer(sq, np.uint8)
    kept = {}                                       # outputs of the 4095 batch, for the 4096 batch to compare with
    forms_run = set()
    for nb in SK_BATCHES:
        idx = order[:nb]
        want_wo = ref.exclusive_scan(ref.num_windows(lens[idx], W, S))
        n_win = int(want_wo[-1])
        want_f = _up(np.concatenate([rows[i] for i in idx]).ravel(), torch.int32)
        want_m = _up(np.concatenate([nfeat[i] for i in idx]), torch.int32)
        text_o = np.frombuffer(b"".join(seqs[i] for i in idx), np.uint8)
        for ranges in (False, True):
            text = _up(text_r if ranges else text_o, torch.uint8)
            so = _up(text_r_off[idx].ravel() if ranges else ref.exclusive_scan(lens[idx]), torch.int64)
            flags = eng.MCQ_BATCH_RANGES if ranges else 0
            for pad in SK_PADS:
                buf = torch.full((text.numel() + 4,), ord("G"), dtype=torch.uint8, device=_dev())
                buf[pad:pad + text.numel()] = text
                assert buf.data_ptr() % 4 == 0
                bases = buf.data_ptr() + pad        # a base pointer that is `pad` bytes off alignment
                win_off = _out(nb + 1, torch.int64)
                db.count_windows(bases, so.data_ptr(), nb, win_off.data_ptr(), flags=flags)
                feats, nf = _out(n_win * s, torch.int32), _out(n_win, torch.int32)
                db.sketch(bases, so.data_ptr(), nb, win_off.data_ptr(), feats.data_ptr(), nf.data_ptr(), flags=flags)
                torch.cuda.synchronize()
                assert np.array_equal(_down(win_off, nb + 1, "win_off"), want_wo), (geom, nb, ranges, pad)
                what = (geom, nb, "ranges" if ranges else "offsets", pad)
                assert bool((feats[n_win * s:] == SENT).all()) and bool((nf[n_win:] == SENT).all()), what
                if not torch.equal(nf[:n_win], want_m):
                    w = int(torch.nonzero(nf[:n_win] != want_m)[0])
                    assert False, (what, "n_feat of window", w, int(nf[w]), int(want_m[w]))
                if not torch.equal(feats[:n_win * s], want_f):      # (the unused slots of a row are 0xFFFFFFFF in want_f)
                    assert False, (what, "features of window",) + _first_row_diff(feats[:n_win * s], want_f, s)
                forms_run.add((nb, ranges, pad))
                if nb == 4095:
                    kept[(ranges, pad)] = (feats[:n_win * s].clone(), nf[:n_win].clone())
                if nb == 4096:                      # both kernels compute the same function: the common prefix, byte for byte
                    f95, m95 = kept[(ranges, pad)]
                    assert m95.numel() == int(want_wo[4095])
                    assert torch.equal(feats[:f95.numel()], f95) and torch.equal(nf[:m95.numel()], m95), what
    assert forms_run == {(nb, r, p) for nb in SK_BATCHES for r in (False, True) for p in SK_PADS}


# ====================================================================================== c. mcq_bucket_features
BK_SMALL = [0, 1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193]
BK_LARGE = [4096 * 17 + 1, 4096 * 2048 + 4097]
BK_SHARDS = [1, 2, 3, 7, 63, 64]
BK_FILLS = ["random", "all-empty", "some-empty", "one-value"]
BK_CASES = [(n, tuple(BK_SHARDS), tuple(BK_FILLS)) for n in BK_SMALL] + [(BK_LARGE[0], (3, 64), tuple(BK_FILLS))] + \
           [(BK_LARGE[1], (ns,), (fill,)) for ns in (3, 64) for fill in BK_FILLS]


def _bk_fill(rng, n, fill):
    f = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    if fill == "all-empty":
        f[:] = EMPTY
    elif fill == "some-empty":
        f[rng.random(n) < 0.3] = EMPTY
    elif fill == "one-value":
        f[:] = 0x1234ABCD
    return f


@pytest.mark.parametrize("n,shards,fills", BK_CASES, ids=["%d-%s-%s" % (n, "x".join(map(str, sh)), "+".join(fi) if len(fi) == 1 else "all")
                                                          for n, sh, fi in BK_CASES])
def test_bucket_features_edges(eng, n, shards, fills):
    """the three-kernel counting sort: counts, bucketed and src_index agree with each other and with the reference, for
    1..64 shards, for sizes around the 4096-feature workgroup tile, the 2048-workgroup cap and the rounded-up tile whose
    last workgroups start behind the input, and for inputs that are empty, all in one shard, or all dropped"""
    assert sorted({c[0] for c in BK_CASES}) == BK_SMALL + BK_LARGE
    assert all(set(c[1]) == set(BK_SHARDS) and set(c[2]) == set(BK_FILLS) for c in BK_CASES if c[0] <= 8193)
    for big in BK_LARGE:
        assert {(ns, fi) for c in BK_CASES if c[0] == big for ns in c[1] for fi in c[2]} == {(a, b) for a in (3, 64) for b in BK_FILLS}
    last_start = []                                 # where the last workgroup starts (mcq_bucket_features' tiling)
    for big in BK_LARGE:
        grid = min((big + 4095) // 4096, 2048)
        tile = ((big + grid - 1) // grid + 255) // 256 * 256
        last_start.append((grid - 1) * tile - big)
    assert last_start[0] == -1                      # one feature in the last workgroup
    assert (BK_LARGE[1] + 4095) // 4096 > 2048 and last_start[1] >= 0      # the grid cap; workgroups that start behind the input
    rng = np.random.default_rng(31 + n)
    for fill in fills:
        f = _bk_fill(rng, n, fill)
        feats = _up(f, torch.int32)
        for ns in shards:
            counts, bucketed, src = _out(ns, torch.int64), _out(n, torch.int32), _out(n, torch.int32)
            eng.bucket_features(feats.data_ptr(), n, ns, counts.data_ptr(), bucketed.data_ptr(), src.data_ptr())
            torch.cuda.synchronize()
            what = (n, ns, fill)
            want_c, want_sets = ref.bucket(f, ns)
            got_c = _down(counts, ns, "counts")
            assert np.array_equal(got_c, want_c), (what, got_c, want_c)
            m = int(want_c.sum())
            got_b, got_s = _down(bucketed, n, "bucketed")[:m], _down(src, n, "src_index")[:m].astype(np.int64)
            assert bool((bucketed[m:] == SENT).all()) and bool((src[m:] == SENT).all()), what    # nothing behind the last segment
            if m == 0:
                continue
            assert int(got_s.max()) < n, what
            seg = np.repeat(np.arange(ns, dtype=np.int64), want_c.astype(np.int64))
            assert np.array_equal(got_b, f[got_s]), what
            assert np.array_equal(ref.owner(got_b, ns), seg), what
            # mcq.h promises no order inside a shard's segment: compare each segment's indices as a set
            assert np.array_equal(np.sort((seg << 32) | got_s), (seg << 32) | np.concatenate(want_sets)), what
            probe = f[rng.integers(0, n, size=64)]
            probe = probe[probe != EMPTY]
            assert [eng.owner(int(v), ns) for v in probe.tolist()] == ref.owner(probe, ns).tolist(), what


def test_bucket_features_rejects_shard_counts_out_of_range(eng):
    feats = _up(np.arange(8, dtype=np.uint32), torch.int32)
    counts, bucketed, src = _out(65, torch.int64), _out(8, torch.int32), _out(8, torch.int32)
    for ns in (0, 65):
        with pytest.raises(eng.McqError) as e:
            eng.bucket_features(feats.data_ptr(), 8, ns, counts.data_ptr(), bucketed.data_ptr(), src.data_ptr())
        assert e.value.code == eng.MCQ_E_ARG
    torch.cuda.synchronize()
    _down(counts, 0, "counts"), _down(bucketed, 0, "bucketed"), _down(src, 0, "src_index")


# ====================================================================================== d. mcq_assemble
AS_LENS = np.array([0, 1, 2, 63, 64, 65, 254], np.uint32)
AS_NLISTS = [0, 1, 63, 64, 65, 8193]
AS_BIG_NSEQS = 8192 * 1025 + 3
G_S1 = (16, 1, 128, 113)            # n_slots = n_win * s: 8191 is prime, so that size needs a sketch of one feature
# (name, geometry, location bytes, paired, ranges, n_lists, exact n_slots or None)
AS_CASES = []
for _i, _nl in enumerate(AS_NLISTS):
    for _j, _lb in enumerate((4, 8)):
        _c = _i + _j
        AS_CASES.append(("lists%d" % _nl, GEOMETRIES[(2 * _i + _j) % 5], _lb, bool(_c & 1), bool(_c & 2), _nl, None))
AS_CASES += [("slots8191", G_S1, 4, False, True, 65, 8191), ("slots8192", (8, 4, 100, 93), 8, True, False, 65, 8192),
             ("slots8193", (1, 3, 20, 20), 4, True, True, 8193, 8193), ("big", (1, 3, 20, 20), 8, False, False, 48, None)]


def _as_reads(geom, rng, n_slots):
    """a few hundred read lengths of mixed window counts; with n_slots: exactly n_slots / s windows"""
    k, s, W, S = geom
    if n_slots is None:
        n_slots = 600 * 16
    assert n_slots % s == 0
    target = n_slots // s
    per = max(2, target // 250)                     # windows of the longest reads
    lens, have = [], 0
    while have < target:
        L = int(rng.integers(0, W + 2 * per * S))
        c = int(ref.num_windows(L, W, S)[0])
        if have + c > target:
            L, c = int(rng.integers(0, W + 1)), 1   # fill up with reads of one window
        lens.append(L); have += c
    return np.array(lens, np.uint64)


@pytest.mark.parametrize("case", AS_CASES, ids=[c[0] + "-%dB" % c[2] for c in AS_CASES])
def test_assemble_edges(eng, case):
    """lists in any order into per-query segments: both location widths, single-end and paired, offsets and ranges, empty
    lists, slots without a list, no list at all, n_slots around the scan tile, and so many slots that the scan of the
    tile sums loops with a carry (1024 threads)"""
    name, geom, loc_bytes, paired, ranges, n_lists, exact_slots = case
    assert {c[2] for c in AS_CASES} == {4, 8} and {c[5] for c in AS_CASES if c[0].startswith("lists")} == set(AS_NLISTS)
    assert {(c[2], c[3], c[4]) for c in AS_CASES} >= {(b, p, r) for b in (4, 8) for p in (False, True) for r in (False, True)}
    assert {c[6] for c in AS_CASES if c[6]} == {8191, 8192, 8193}
    k, s, W, S = geom
    rng = np.random.default_rng(4000 + AS_CASES.index(case))
    db = _empty_db(eng, geom, flags=eng.MCQ_DB_LOCS_64 if loc_bytes == 8 else 0)
    assert db.loc_bytes() == loc_bytes
    if name == "big":
        seq_len = np.zeros(AS_BIG_NSEQS, np.uint64)
    else:
        seq_len = _as_reads(geom, rng, exact_slots)
        assert 100 <= len(seq_len) <= 2000 and len(set(seq_len.tolist())) > 50
    n_seqs = len(seq_len)
    nq = n_seqs // 2 if paired else n_seqs
    win_off = ref.exclusive_scan(ref.num_windows(seq_len, W, S))
    n_slots = int(win_off[-1]) * s
    if exact_slots:
        assert n_slots == exact_slots
    if name == "big":                               # a few dozen lists over the whole range, at tile edges among others
        assert n_slots // SCAN_TILE > 1024
        slots = np.unique(np.concatenate([np.linspace(0, n_slots - 1, n_lists - 8).astype(np.int64),
                                          np.array([SCAN_TILE - 1, SCAN_TILE, SCAN_TILE * 1024 - 1, SCAN_TILE * 1024,
                                                    SCAN_TILE * 1024 + 1, SCAN_TILE * 1025, n_slots - 2, 1])]))
        slots = rng.permutation(slots)
        n_lists = len(slots)
        assert 24 <= n_lists <= 64 and slots.min() == 0 and slots.max() == n_slots - 1
    else:
        assert n_slots >= n_lists and np.diff(win_off.astype(np.int64)).max() > 1       # ragged win_off
        # a subset, in shuffled order; where there is room, the last window gets no list: loc_off[nq] behind empty slots
        slots = rng.choice(n_slots - s if n_lists <= n_slots - s else n_slots, size=n_lists, replace=False)
    lens = rng.choice(AS_LENS, size=n_lists).astype(np.uint32)
    if n_lists >= 63:
        lens[:len(AS_LENS)] = AS_LENS               # every length at least once, and two long lists
        lens[len(AS_LENS):len(AS_LENS) + 2] = 5000
        rng.shuffle(lens)
        assert any(int(lens[g:g + 64].sum()) % 64 for g in range(0, n_lists, 64))      # a group of 64 lists with a ragged total
    total = int(lens.astype(np.int64).sum())
    i = np.arange(total, dtype=np.uint64)           # a running counter (in both halves of a 64-bit word): every misplaced word shows
    src = (i if loc_bytes == 4 else (i << np.uint64(32)) | i).astype(np.uint32 if loc_bytes == 4 else np.uint64)
    want_dst, want_off, want_len = ref.assemble(lens, slots, n_slots, src, seq_len, win_off, s, paired)

    ldt = torch.int32 if loc_bytes == 4 else torch.int64
    seq_off = _up(_layout(seq_len, ranges, rng), torch.int64)
    bases = torch.zeros(1, dtype=torch.uint8, device=_dev())            # mcq_assemble reads seq_off only
    d_len, d_slot, d_src, d_wo = _up(lens, torch.int32), _up(slots.astype(np.uint32), torch.int32), _up(src, ldt), _up(win_off, torch.int64)
    loc_off, qlen, dst = _out(nq + 1, torch.int64), _out(nq, torch.int32), _out(total, ldt)
    none_if_empty = lambda t: t.data_ptr() if n_lists else None         # with no list the list arrays may be NULL
    db.assemble(n_lists, none_if_empty(d_len), none_if_empty(d_slot), n_slots, none_if_empty(d_src), bases.data_ptr(),
                seq_off.data_ptr(), n_seqs, paired, d_wo.data_ptr(), loc_off.data_ptr(), qlen.data_ptr(), dst.data_ptr(),
                flags=eng.MCQ_BATCH_RANGES if ranges else 0)
    torch.cuda.synchronize()
    got_off, got_len, got_dst = _down(loc_off, nq + 1, "loc_off"), _down(qlen, nq, "query_len"), _down(dst, total, "dst_locs")
    assert np.array_equal(got_off, want_off), (case, np.nonzero(got_off != want_off)[0][:3])
    assert np.array_equal(got_len, want_len), (case, np.nonzero(got_len != want_len)[0][:3])
    bad = np.nonzero(got_dst != want_dst)[0]
    assert len(bad) == 0, (case, "first misplaced words at", bad[:3], got_dst[bad[:3]], want_dst[bad[:3]])
    assert int(want_off[-1]) == total


# ====================================================================================== e. mcq_lookup_count / _gather
LK_LENS = [1, 7, 8, 14, 15, 16, 100, 254]
LK_N = [1, 63, 64, 65, 257, 1000]
LK_KEYS = 400


@functools.lru_cache(maxsize=None)
def _lk_table():
    rng = np.random.default_rng(8)
    keys = np.unique(rng.integers(0, EMPTY, size=LK_KEYS, dtype=np.uint64).astype(np.uint32))
    assert len(keys) == LK_KEYS
    lens = np.array([LK_LENS[i % len(LK_LENS)] for i in range(LK_KEYS)], np.int64)
    off = ref.exclusive_scan(lens)
    # the location says which list it belongs to and where: target = index of the key, window = position in the list
    locs = (np.repeat(np.arange(LK_KEYS, dtype=np.uint64), lens) << np.uint64(32)) | \
           (np.arange(int(off[-1]), dtype=np.uint64) - np.repeat(off[:-1], lens))
    return keys, lens, off, locs


@pytest.mark.parametrize("n_shards", [1, 3])
@pytest.mark.parametrize("flag_names", [(), ("MCQ_DB_LOCS_64",), ("MCQ_DB_LOCS_GW",), ("MCQ_DB_SLOTS_16",),
                                        # (lists this long make the handle pick 16-B slots: the lists of up to 7 / 14
                                        # locations inside a 64-B bucket need the flag)
                                        ("MCQ_DB_BUCKETS_64",), ("MCQ_DB_LOCS_64", "MCQ_DB_BUCKETS_64")],
                         ids=lambda f: "+".join(f) if f else "default")
def test_lookup_gather_with_kept_starts(eng, flag_names, n_shards):
    """the path of the sharded loop: mcq_lookup_count keeps the list starts, mcq_lookup_gather copies from them -- the
    table's lengths (0 for absent, foreign and reserved features), the table's lists in probe order, and the same bytes
    as the gather that probes again; groups of 64 features with no location at all and with 64 x 254 of them"""
    keys, lens, off, locs = _lk_table()
    dbflags = 0
    for f in flag_names:
        dbflags |= getattr(eng, f)
    tgt_windows = np.full(LK_KEYS, max(LK_LENS), np.uint32)
    gw_off = ref.exclusive_scan(tgt_windows)
    own = ref.owner(keys, n_shards)
    absent = np.setdiff1d(np.random.default_rng(9).integers(0, EMPTY, size=64, dtype=np.uint64).astype(np.uint32), keys)
    widths = set()
    for sid in range(n_shards):
        db = eng.Database(keys, off, locs, np.arange(LK_KEYS, dtype=np.uint32), n_shards=n_shards, shard_id=sid, flags=dbflags,
                          tgt_windows=tgt_windows)
        widths.add(db.loc_bytes())
        assert db.loc_bytes() == (8 if "MCQ_DB_LOCS_64" in flag_names else 4)
        assert (db.layout()["loc_format"] == eng.MCQ_LOC_GLOBAL_WINDOW) == ("MCQ_DB_LOCS_GW" in flag_names)
        if len(flag_names) and flag_names[-1] in ("MCQ_DB_SLOTS_16", "MCQ_DB_BUCKETS_64"):
            assert db.layout()["bucket_bytes"] == (16 if "MCQ_DB_SLOTS_16" in flag_names else 64)
        ldt = torch.int32 if db.loc_bytes() == 4 else torch.int64
        mine, foreign = np.nonzero(own == sid)[0], np.nonzero(own != sid)[0]
        longest = mine[lens[mine] == 254]
        assert len(longest) and (n_shards == 1) == (len(foreign) == 0)
        rng = np.random.default_rng(60 + sid)
        for n in LK_N:
            # present keys (with repeats), absent ones, the reserved value, keys of another shard
            pool = np.concatenate([keys[rng.choice(mine, size=n)], absent[rng.integers(0, len(absent), size=n)],
                                   np.full(n, EMPTY, np.uint32), keys[rng.choice(foreign, size=n)] if len(foreign) else absent[:1]])
            kind = rng.choice([0, 0, 0, 1, 2, 3], size=n) if len(foreign) else rng.choice([0, 0, 0, 1, 2], size=n)
            probe = pool[np.minimum(kind * n + np.arange(n), len(pool) - 1)].astype(np.uint32)
            if n == 1000:
                nothing = np.concatenate([absent[:30], np.full(10, EMPTY, np.uint32), keys[foreign[:24]] if len(foreign) else absent[30:54]])
                probe[128:128 + 64] = nothing                           # a 64-aligned group without a single location
                probe[192:256] = keys[rng.choice(longest, size=64)]     # and one of 64 lists of 254: 64 rounds of the copy loop
            at = np.searchsorted(keys, probe)
            at[at == LK_KEYS] = 0
            hit = (keys[at] == probe) & (own[at] == sid)
            want_len = np.where(hit, lens[at], 0)
            if n == 1000:
                assert want_len[128:192].sum() == 0 and want_len[192:256].sum() == 64 * 254 and (kind[:128] == 3).any() == bool(len(foreign))
            want = np.concatenate([locs[int(off[a]):int(off[a + 1])] for a in at[hit]] + [np.zeros(0, np.uint64)])
            total = int(want_len.sum())
            d_probe = _up(probe, torch.int32)
            len_a, len_b, starts = _out(n, torch.int32), _out(n, torch.int32), _out(n, torch.int64)
            db.lookup_count(d_probe.data_ptr(), n, len_a.data_ptr(), starts.data_ptr())
            db.lookup_count(d_probe.data_ptr(), n, len_b.data_ptr(), None)
            out_off = _up(ref.exclusive_scan(want_len), torch.int64)
            kept, again = _out(total, ldt), _out(total, ldt)
            db.lookup_gather(d_probe.data_ptr(), n, out_off.data_ptr(), kept.data_ptr(), len_a.data_ptr(), starts.data_ptr())
            db.lookup_gather(d_probe.data_ptr(), n, out_off.data_ptr(), again.data_ptr())
            torch.cuda.synchronize()
            what = (flag_names, n_shards, sid, n)
            assert np.array_equal(_down(len_a, n, "list_len"), want_len), what
            assert np.array_equal(_down(len_b, n, "list_len"), want_len), what
            _down(starts, n, "list_src")
            got_kept, got_again = _down(kept, total, "out_locs"), _down(again, total, "out_locs")
            assert np.array_equal(ref.decode_native(db, got_kept, gw_off), want), what
            assert np.array_equal(ref.decode_native(db, got_again, gw_off), want), what
            assert got_kept.tobytes() == got_again.tobytes(), what
    assert widths == ({8} if "MCQ_DB_LOCS_64" in flag_names else {4})
