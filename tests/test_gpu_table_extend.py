"""mcq_table_extend_* (include/mcq.h) through the Python mirror: a table built from the targets A, handed back as the triples its
shard files would hold, and extended by the targets B, against mcq_build_table of A and B together and against
dbbuild_torch.build_table, the second implementation -- the reference's `modify` appends to the buckets of the ranks, so a
database built from A and extended by B holds what one built from A and B holds (src/sketch_database.h:1079-1097)."""
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_A = 7                    # targets 0..6 are the old ones: at P = 8 rank 7 owns no old target
PS = (1, 2, 3, 8)
# copies of three repeat elements per target: with them every P in PS has, at max_locs 2 and 3, a (feature, rank) group that the
# old targets fill exactly, and one that they leave one short, with new entries waiting behind (asserted in kinds())
COPIES = ([0, 0, 0, 0, 1, 0, 1, 2, 0, 2, 1, 0], [0, 0, 0, 1, 0, 0, 0, 1, 2, 0, 2, 0], [0, 1, 2, 3, 0, 0, 0, 0, 2, 1, 1, 3])
ELEMENT_WINDOWS, STRIDE = 6, 113


def make_world():
    """12 genomes of 30-60 kb, 3 species of 4 strains 2 % apart (made on the CPU: the same bases everywhere), and three repeat
    elements of 6 windows written over them on the window grid, so that the windows inside a copy are the same in every copy"""
    synth = importlib.import_module("metacache-mpi_amd.synth")
    cpu = torch.device("cpu")
    bases, off, _ = synth.make_genomes(3, 4, 30_000, 60_000, 0.02, seed=41, device=cpu)
    bases = bases.clone()
    g = torch.Generator(device=cpu); g.manual_seed(42)
    acgt = torch.tensor([65, 67, 71, 84], dtype=torch.uint8)
    for e, copies in enumerate(COPIES):
        element = acgt[torch.randint(0, 4, (ELEMENT_WINDOWS * STRIDE + 15,), generator=g)]
        for t, c in enumerate(copies):
            for j in range(c):
                at = int(off[t]) + STRIDE * (10 + 40 * e + 12 * j)
                assert at + len(element) <= int(off[t + 1])
                bases[at:at + len(element)] = element
    return bases, off


@pytest.fixture(scope="module")
def world():
    eng = importlib.import_module("metacache-mpi_amd.engine")
    bases, off = make_world()
    dev = torch.device("cuda", 0)
    return eng, bases.to(dev), off.to(dev)


def build(eng, bases, off, t0, t1, P, max_locs=0, flags=0):
    """mcq_build_table of targets t0..t1 -> (keys, list_off, locs, win_off) on the host"""
    sub = (off[t0:t1 + 1] - off[t0]).contiguous()
    seq = bases[int(off[t0]):int(off[t1])].contiguous()
    t = eng.Table(seq.data_ptr(), sub.data_ptr(), t1 - t0, emulate_ranks=P, max_locs=max_locs, flags=flags, device=0)
    out = t.to_host()
    t.close()
    return out


def rank_files(keys, off, locs, P):
    """the triples the P shard files of a table hold, each in file order: key by key, a list in (target, window) order"""
    feat = np.repeat(keys, np.diff(off.astype(np.int64)))
    tgt, win = (locs >> np.uint64(32)).astype(np.uint32), (locs & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return [(feat[tgt % P == r], tgt[tgt % P == r], win[tgt % P == r]) for r in range(P)]


def extend(eng, bases, off, old, n_a, n_all, P, max_locs=0, flags=0, chunk=1 << 20, order=None, expected=None, device_chunks=False):
    """old = (keys, list_off, locs, win_off) of the table of targets 0..n_a: its files, chunk by chunk, then targets n_a..n_all"""
    keys, loff, locs, win_off = old
    files = rank_files(keys, loff, locs, P)
    x = eng.TableExtend(np.diff(win_off.astype(np.int64)).astype(np.uint32), n_ranks=P, max_locs=max_locs, flags=flags,
                        expected_old_locations=len(locs) if expected is None else expected, device=0)
    for r in (range(P) if order is None else order):
        f, t, w = files[r]
        for c, i in enumerate(range(0, len(f), chunk)):
            if device_chunks and c % 2:
                d = [torch.from_numpy(np.ascontiguousarray(a[i:i + chunk]).view(np.int32).copy()).cuda() for a in (f, t, w)]
                x.add(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), n=len(d[0]))
            else:
                x.add(f[i:i + chunk], t[i:i + chunk], w[i:i + chunk])
    sub = (off[n_a:n_all + 1] - off[n_a]).contiguous()
    seq = bases[int(off[n_a]):int(off[n_all])].contiguous()
    t = x.finish(seq.data_ptr() if n_all > n_a else None, sub.data_ptr() if n_all > n_a else None, n_all - n_a)
    assert x.h is None
    out = t.to_host()
    t.close()
    return out


def same(a, b):
    return all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


_torch_tables = {}


def torch_table(bases, off, P, max_locs, overpop=False):
    """dbbuild_torch.build_table of all targets, once per (P, max_locs, flag)"""
    key = (P, max_locs, overpop)
    if key not in _torch_tables:
        dbbuild = importlib.import_module("dbbuild_torch")
        k, o, l, w = dbbuild.build_table(bases, off, emulate_ranks=P, maxlocs=max_locs, remove_overpopulated=overpop)
        _torch_tables[key] = (k.cpu().numpy().astype(np.uint32), o.cpu().numpy().astype(np.uint64), l.cpu().numpy().astype(np.uint64),
                              w.cpu().numpy().astype(np.uint64))
    return _torch_tables[key]


def kinds(table254, n_a, P, M):
    """of the (feature, rank) groups of the untruncated table of all targets: how many the old targets fill exactly (or more) with
    new entries behind, leave one short with new entries behind, hold alone, and do not hold at all"""
    keys, off, locs, _ = table254
    feat = np.repeat(keys.astype(np.int64), np.diff(off.astype(np.int64)))
    tgt = (locs >> np.uint64(32)).astype(np.int64)
    group = feat * P + tgt % P
    ids, inv = np.unique(group, return_inverse=True)
    c_a = np.bincount(inv, weights=(tgt < n_a), minlength=len(ids)).astype(np.int64)
    c_b = np.bincount(inv, weights=(tgt >= n_a), minlength=len(ids)).astype(np.int64)
    assert (c_a + c_b).max() < 254
    return (int(((c_a >= M) & (c_b > 0)).sum()), int(((c_a == M - 1) & (c_b > 0)).sum()), int(((c_a > 0) & (c_b == 0)).sum()),
            int(((c_a == 0) & (c_b > 0)).sum()))


@pytest.mark.parametrize("max_locs", [254, 2, 3])
@pytest.mark.parametrize("P", PS)
def test_extended_table_equals_the_one_shot_build(world, P, max_locs):
    """A = targets 0..6 built alone, its triples and then B = targets 7..11 through the extender: keys, list_off, locations and
    win_off of mcq_build_table(A + B), and of dbbuild_torch.build_table(A + B).  At max_locs 2 and 3 the input holds groups that
    are exactly full, one short of full, only in A and only in B"""
    eng, bases, off = world
    n_all = off.numel() - 1
    assert n_all == 12
    if max_locs != 254:
        found = kinds(torch_table(bases, off, P, 254), N_A, P, max_locs)
        print("P %d max_locs %d: groups full / one short / only old / only new: %s" % (P, max_locs, found))
        assert min(found) > 0, found
    one_shot = build(eng, bases, off, 0, n_all, P, max_locs)
    old = build(eng, bases, off, 0, N_A, P, max_locs)
    got = extend(eng, bases, off, old, N_A, n_all, P, max_locs)
    assert len(got[0]) > 10000 and len(got[2]) > len(old[2])
    assert same(got, one_shot)
    assert same(got, torch_table(bases, off, P, max_locs))


def test_fewer_old_targets_than_ranks_and_a_new_sequence_shorter_than_k(world):
    """2 old targets at P = 8: six files without a location, whose ranks B fills; and B with a sequence of 10 bases in its middle,
    which becomes a target of one window without a feature"""
    eng, bases, off = world
    dev = bases.device
    got = extend(eng, bases, off, build(eng, bases, off, 0, 2, 8), 2, 12, 8)
    assert same(got, build(eng, bases, off, 0, 12, 8))
    cut = int(off[9])
    b2 = torch.cat([bases[:cut], bases[cut:cut + 10], bases[cut:]])
    o2 = torch.cat([off[:10], off[9:10] + 10, off[10:] + 10]).to(dev)
    assert o2.numel() == 14 and int(o2[10] - o2[9]) == 10
    for P in (1, 3):
        got = extend(eng, b2, o2, build(eng, b2, o2, 0, N_A, P), N_A, 13, P)
        assert same(got, build(eng, b2, o2, 0, 13, P))
        assert np.diff(got[3].astype(np.int64))[9] == 1 and not ((got[2] >> np.uint64(32)) == 9).any()      # one window, no feature


def test_no_new_target_gives_the_old_table_back(world):
    eng, bases, off = world
    for P, M in ((1, 254), (3, 3)):
        old = build(eng, bases, off, 0, N_A, P, M)
        assert same(extend(eng, bases, off, old, N_A, N_A, P, M), old)


@pytest.mark.parametrize("P", (1, 3))
def test_remove_overpopulated_given_only_to_the_extension(world, P):
    """A built without the flag, the extension with it, at max_locs 3: the one-shot build of A + B with the flag (features with
    more than 2 locations over all ranks go), which drops keys the unflagged build keeps"""
    eng, bases, off = world
    flag = eng.MCQ_BUILD_REMOVE_OVERPOPULATED
    got = extend(eng, bases, off, build(eng, bases, off, 0, N_A, P, 3), N_A, 12, P, 3, flags=flag)
    assert same(got, build(eng, bases, off, 0, 12, P, 3, flags=flag))
    assert same(got, torch_table(bases, off, P, 3, overpop=True))
    assert len(got[0]) < len(torch_table(bases, off, P, 3)[0])


@pytest.mark.parametrize("P", (2, 8))
def test_a_lower_limit_in_the_extension_shrinks_the_old_buckets(world, P):
    """A built at max_locs 4, extended at 2: per (feature, rank) the first 2 old entries, then the new ones, cut at 2, then the
    ranks merged -- rules 3 and 4 restated in NumPy from A's table and from the new targets' entries in the untruncated table of
    all targets.  No file of the reference pins this case (its golden databases were built in one go): the restatement is the check"""
    eng, bases, off = world
    N = 2
    old = build(eng, bases, off, 0, N_A, P, 4)
    got = extend(eng, bases, off, old, N_A, 12, P, N)
    full = torch_table(bases, off, P, 254)

    def entries(table, keep):
        keys, loff, locs, _ = table
        feat = np.repeat(keys.astype(np.int64), np.diff(loff.astype(np.int64)))
        tgt = (locs >> np.uint64(32)).astype(np.int64)
        m = keep(tgt)
        return feat[m], tgt[m], locs[m]
    fa, ta, la = entries(old, lambda t: t >= 0)
    fb, tb, lb = entries(full, lambda t: t >= N_A)
    feat, tgt, loc = np.concatenate([fa, fb]), np.concatenate([ta, tb]), np.concatenate([la, lb])
    is_new = np.concatenate([np.zeros(len(fa), np.int64), np.ones(len(fb), np.int64)])
    group = feat * P + tgt % P
    order = np.lexsort((loc, is_new, group))                  # per group: old entries in their order, then the new ones in theirs
    group, feat, loc = group[order], feat[order], loc[order]
    start = np.flatnonzero(np.r_[True, group[1:] != group[:-1]])
    pos = np.arange(len(group)) - np.repeat(start, np.diff(np.r_[start, len(group)]))
    feat, loc = feat[pos < N], loc[pos < N]
    order = np.lexsort((loc, feat))                            # the ranks' lists of a feature merged into (target, window) order
    feat, loc = feat[order], loc[order]
    keys, counts = np.unique(feat, return_counts=True)
    want_off = np.zeros(len(keys) + 1, np.uint64); want_off[1:] = np.cumsum(counts)
    assert np.unique(fa * P + ta % P, return_counts=True)[1].max() > N      # an old bucket is longer than the new limit: something is shrunk
    assert np.array_equal(got[0], keys.astype(np.uint32)) and np.array_equal(got[1], want_off) and np.array_equal(got[2], loc)
    assert np.array_equal(got[3], full[3])


def test_shuffled_files_small_chunks_and_a_buffer_that_has_to_grow(world):
    """the files in another order, in chunks of 1000 triples, every second chunk as device pointers, and the pair buffer sized for
    a tenth of what arrives: the same table"""
    eng, bases, off = world
    P = 3
    old = build(eng, bases, off, 0, N_A, P, 3)
    want = build(eng, bases, off, 0, 12, P, 3)
    assert len(old[2]) > 20000
    assert same(extend(eng, bases, off, old, N_A, 12, P, 3, chunk=1000, order=(2, 0, 1), device_chunks=True), want)
    assert same(extend(eng, bases, off, old, N_A, 12, P, 3, chunk=1777, order=(1, 2, 0), expected=len(old[2]) // 10), want)


def test_triples_the_database_does_not_have_are_refused(world):
    eng, bases, off = world
    one = np.ones(1, np.uint32)
    for f, t, w in ((7, 2, 0), (7, 0, 5), (0xFFFFFFFF, 0, 0)):
        x = eng.TableExtend(np.array([5, 5], np.uint32), n_ranks=2, device=0)
        with pytest.raises(eng.McqError) as e:
            x.add(one * f, one * t, one * w)
        assert e.value.code == eng.MCQ_E_ARG
        x.close()
    with pytest.raises(eng.McqError):
        eng.TableExtend(np.array([5], np.uint32), k=17, device=0)
