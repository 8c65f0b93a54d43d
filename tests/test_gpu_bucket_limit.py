"""mcq_bucket_limit alone (csrc/mcq_bucket_limit.hip): the query-time bucket rules on a chunk of triples against the NumPy
statement of tests/bucket_limit_ref.py, array for array plus the three counts, with host pointers and with device pointers.

The kernels work on tiles of TILE = 2048 triples (a workgroup of 4 waves, each wave 512 contiguous triples in steps of 64),
so the chunk below puts runs across every 64, 512 and 2048 boundary, one on purpose across the first tile boundary, and one
longer than two tiles (a tile without any run head)."""
import functools
import importlib

import numpy as np
import pytest
import torch

import bucket_limit_ref as ref

pytestmark = pytest.mark.gpu
TILE = 2048          # BL_TILE of csrc/mcq_bucket_limit.hip
K = 40               # the N the run lengths are drawn around


def _eng():
    return importlib.import_module("metacache-mpi_amd.engine")


def _triples(lengths, seed):
    lengths = np.asarray(lengths, np.int64)
    rng = np.random.default_rng(seed)
    ids = (np.arange(len(lengths), dtype=np.uint64) * np.uint64(2654435761) + np.uint64(12345)) % np.uint64(0xFFFFFFFF)   # distinct: neighbours differ
    feat = np.repeat(ids.astype(np.uint32), lengths)
    n = int(lengths.sum())
    return feat, rng.integers(0, 1 << 20, n, dtype=np.uint32), np.arange(n, dtype=np.uint32)     # (win = index: an order mistake shows)


@functools.lru_cache(maxsize=None)
def _big():
    """about 70 000 triples: a run of 1000 from 1948 to 2948 (across the first tile boundary), one of 5000 (a whole tile inside
    it), then lengths drawn from {1, 2, K-1, K, K+1, 63, 64, 65, 254, 255, 256, 1000}; the first run starts at 0, the last
    (256 long) ends at n - 1"""
    rng = np.random.default_rng(7)
    head = [1000, 254, 255, 256, 65, 64] + [2] * 27
    assert sum(head) == TILE - 100
    lengths = head + [1000, 5000]
    pool = [1, 2, K - 1, K, K + 1, 63, 64, 65, 254, 255, 256, 1000]
    while sum(lengths) < 70000:
        lengths.append(int(rng.choice(pool)))
    lengths.append(256)
    assert (sum(lengths) % 64, sum(lengths) % TILE) != (0, 0)
    return _triples(lengths, 11)


def _run(feat, tgt, win, keep_first, remove_above, device_ptrs):
    """device_ptrs: False = host arrays, True = device arrays, "ws" = device arrays and the caller's scratch (mcq_bucket_limit_ws)"""
    eng = _eng()
    if not device_ptrs:
        return eng.bucket_limit(feat, tgt, win, keep_first, remove_above)
    dev = torch.device("cuda", 0)
    d = [torch.from_numpy(x.view(np.int32).copy()).to(dev) for x in (feat, tgt, win)]
    st = torch.cuda.current_stream(dev).cuda_stream
    if device_ptrs == "ws":
        nb = eng.bucket_limit_scratch_bytes(len(feat))
        scratch = torch.full((nb + 256,), 0x5A, dtype=torch.uint8, device=dev)          # (dirty on purpose; the tail is a guard)
        c = eng.bucket_limit_ws(*(x.data_ptr() if x.numel() else 0 for x in d), len(feat), keep_first, remove_above, scratch.data_ptr(), nb, stream=st)
        torch.cuda.synchronize(dev)
        assert bool((scratch[nb:] == 0x5A).all())
        return tuple(x[:int(c[0])].cpu().numpy().view(np.uint32) for x in d) + (int(c[1]), int(c[2]))
    no, ns, nr = eng.bucket_limit(*(x.data_ptr() if x.numel() else 0 for x in d), keep_first, remove_above, n=len(feat), stream=st)
    torch.cuda.synchronize(dev)                          # (the caller synchronises before reading the counts)
    k = int(no.value)
    return tuple(x[:k].cpu().numpy().view(np.uint32) for x in d) + (int(ns.value), int(nr.value))


def _check(feat, tgt, win, keep_first, remove_above, device_ptrs):
    want = ref.bucket_limit(feat, tgt, win, keep_first, remove_above)
    got = _run(feat, tgt, win, keep_first, remove_above, device_ptrs)
    assert got[3:] == want[3:], (got[3:], want[3:])
    assert len(got[0]) == len(want[0])
    for g, w in zip(got[:3], want[:3]):
        assert np.array_equal(g, w)


RULES = [(1, 0), (K, 0), (255, 0),                 # shrink alone
         (0, K - 1), (0, 1), (0, 999),             # removal alone
         (K, 64), (1, 253), (255, 255)]            # both


@pytest.mark.parametrize("device_ptrs", [False, True, "ws"])
@pytest.mark.parametrize("keep_first,remove_above", RULES)
def test_big_chunk_equals_the_numpy_rule(keep_first, remove_above, device_ptrs):
    _check(*_big(), keep_first, remove_above, device_ptrs)


@pytest.mark.parametrize("device_ptrs", [False, True])
@pytest.mark.parametrize("length", [1, 5, 64, 300, TILE, 3 * TILE + 17])
def test_one_run_only(length, device_ptrs):
    f, t, w = _triples([length], 3)
    for keep_first, remove_above in ((K, 0), (0, K), (255, 4096), (1, 0)):
        _check(f, t, w, keep_first, remove_above, device_ptrs)


@pytest.mark.parametrize("device_ptrs", [False, True, "ws"])
def test_runs_at_both_ends_and_sizes_around_the_tile(device_ptrs):
    for lengths in ([300, 1, 1, 300], [1, 300, 1], [TILE - 1, 2, TILE - 1], [TILE], [TILE, TILE], [63, 1, 64, 1, 65], [K + 1] * 60):
        f, t, w = _triples(lengths, 5)
        _check(f, t, w, K, 0, device_ptrs)
        _check(f, t, w, K, 299, device_ptrs)


@pytest.mark.parametrize("device_ptrs", [False, True])
def test_no_triples(device_ptrs):
    e = np.zeros(0, np.uint32)
    got = _run(e, e, e, K, K, device_ptrs)
    assert len(got[0]) == 0 and got[3:] == (0, 0)


def test_both_rules_off_leave_the_arrays_untouched():
    eng = _eng()
    f, t, w = _big()
    of, ot, ow, ns, nr = eng.bucket_limit(f, t, w, 0, 0)
    assert np.array_equal(of, f) and np.array_equal(ot, t) and np.array_equal(ow, w) and (ns, nr) == (0, 0)
    dev = torch.device("cuda", 0)
    d = [torch.from_numpy(x.view(np.int32).copy()).to(dev) for x in (f, t, w)]
    no, ns, nr = eng.bucket_limit(*(x.data_ptr() for x in d), 0, 0, n=len(f), stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    assert (no.value, ns.value, nr.value) == (len(f), 0, 0)
    for x, h in zip(d, (f, t, w)):
        assert np.array_equal(x.cpu().numpy().view(np.uint32), h)


def test_bad_arguments():
    eng = _eng()
    f, t, w = _triples([3, 3], 1)
    with pytest.raises(eng.McqError) as e:
        eng.bucket_limit(f, t, w, 256, 0)                                        # keep_first > 255
    assert e.value.code == eng.MCQ_E_ARG
    with pytest.raises(eng.McqError) as e:
        eng.bucket_limit(0, 0, 0, K, 0, n=6)                                     # null arrays with n > 0
    assert e.value.code == eng.MCQ_E_ARG
