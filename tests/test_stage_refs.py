"""The plain references of tests/stage_refs.py against the oracle and against cases small enough to work out by hand
(CPU only): a wrong reference must not be able to hide a wrong kernel in tests/test_gpu_stage_edges.py."""
import numpy as np
import pytest

import stage_refs as ref
from oracle import mc_oracle as orc

# (k, s, W, S) of tests/test_gpu_stage_edges.py
GEOMETRIES = [(16, 16, 128, 113), (12, 8, 64, 53), (16, 16, 128, 64), (8, 4, 100, 93), (1, 3, 20, 20), (16, 16, 128, 1)]


@pytest.mark.parametrize("geom", GEOMETRIES)
def test_windows_equal_the_oracle(geom):
    _, _, W, S = geom
    lens = np.arange(0, 1201)
    counts = ref.num_windows(lens, W, S)
    assert counts.dtype == np.uint64
    for n in lens.tolist():
        want = orc.windows(n, W, S)
        assert ref.windows(n, W, S) == want, (geom, n)
        assert int(counts[n]) == len(want), (geom, n)


def test_num_windows_beyond_32_bits():
    """2^33 bases at stride 1 have more than 2^32 windows: the count is a 64-bit number"""
    n = 1 << 33
    assert int(ref.num_windows(n, 128, 1)[0]) == (n - 128 + 1) + 1              # the full windows and the short one behind
    assert int(ref.num_windows(n, 128, 113)[0]) == (n - 128) // 113 + 2
    assert int(ref.num_windows(n, 20, 20)[0]) == (n - 20) // 20 + 2


def test_hash_equals_the_oracle():
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.integers(0, 1 << 32, size=10_000, dtype=np.uint64).astype(np.uint32),
                        np.array([0, 1, 0xFFFFFFFE], np.uint32)])
    got = ref.tmh(x)
    assert got.dtype == np.uint64 and int(got.max()) < (1 << 32)
    assert got.tolist() == [orc.tmh(int(v)) for v in x.tolist()]
    for ns in (1, 3, 64):
        assert ref.owner(x, ns).tolist() == [(orc.tmh(int(v)) * ns) >> 32 for v in x.tolist()]
    assert ref.owner(np.array([0xFFFFFFFF], np.uint32), 5).tolist() == [-1]


def test_exclusive_scan_by_hand():
    assert ref.exclusive_scan([]).tolist() == [0]
    assert ref.exclusive_scan([4]).tolist() == [0, 4]
    out = ref.exclusive_scan(np.array([3, 0, 2, 0xFFFFFFFF, 1], np.uint32))
    assert out.dtype == np.uint64
    assert out.tolist() == [0, 3, 3, 5, 5 + 0xFFFFFFFF, 6 + 0xFFFFFFFF]


def test_bucket_by_hand():
    #                 0  1  2  3           4      5           6  7  8           9           10  11
    f = np.array([0, 1, 2, 0xFFFFFFFF, 12345, 0xFFFFFFFE, 7, 7, 0xFFFFFFFF, 0x80000000, 99, 3000000000], np.uint32)
    # tmh: 0, 31251ba7, 66a79298, -, 68296f19, 477a6db9, 08d5d6f3, 08d5d6f3, -, 3d5a6175, 9c801c47, edd70e4e; thirds of 2^32
    # end at 55555555 and aaaaaaaa
    assert ref.owner(f, 3).tolist() == [0, 0, 1, -1, 1, 0, 0, 0, -1, 0, 1, 2]
    counts, sets = ref.bucket(f, 3)
    assert counts.tolist() == [6, 3, 1]
    assert [s.tolist() for s in sets] == [[0, 1, 5, 6, 7, 9], [2, 4, 10], [11]]
    counts, sets = ref.bucket(f, 1)
    assert counts.tolist() == [10] and sets[0].tolist() == [0, 1, 2, 4, 5, 6, 7, 9, 10, 11]
    counts, sets = ref.bucket(np.zeros(0, np.uint32), 4)
    assert counts.tolist() == [0, 0, 0, 0] and [len(s) for s in sets] == [0, 0, 0, 0]
    counts, sets = ref.bucket(np.full(5, 0xFFFFFFFF, np.uint32), 2)
    assert counts.tolist() == [0, 0] and [len(s) for s in sets] == [0, 0]


def test_assemble_by_hand():
    s = 2
    seq_len = [5, 0, 7, 3]
    win_off = [0, 2, 3, 5, 6]                   # 6 windows, 12 feature slots
    src_slot = [7, 0, 11, 4, 2]
    list_len = [2, 3, 0, 1, 2]
    src_locs = np.array([10, 11, 20, 21, 22, 30, 40, 41], np.uint32)
    # slot lengths 3 . 2 . 1 . . 2 . . . 0  ->  slot offsets 0 3 3 5 5 6 6 6 8 8 8 8 | 8
    dst, loc_off, qlen = ref.assemble(list_len, src_slot, 12, src_locs, seq_len, win_off, s, paired=False)
    assert dst.dtype == np.uint32 and dst.tolist() == [20, 21, 22, 40, 41, 30, 10, 11]
    assert loc_off.tolist() == [0, 5, 6, 8, 8]          # first slots 0, 4, 6, 10
    assert qlen.tolist() == [5, 0, 7, 3]
    dst, loc_off, qlen = ref.assemble(list_len, src_slot, 12, src_locs.astype(np.uint64), seq_len, win_off, s, paired=True)
    assert dst.dtype == np.uint64 and dst.tolist() == [20, 21, 22, 40, 41, 30, 10, 11]
    assert loc_off.tolist() == [0, 6, 8]                # first slots 0, 6
    assert qlen.tolist() == [5, 10]
    # no list at all: every segment is empty
    dst, loc_off, qlen = ref.assemble([], [], 12, np.zeros(0, np.uint32), seq_len, win_off, s, paired=False)
    assert len(dst) == 0 and loc_off.tolist() == [0, 0, 0, 0, 0] and qlen.tolist() == [5, 0, 7, 3]
