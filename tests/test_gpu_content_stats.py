"""mcq_content_stats_* alone (csrc/mcq_content_stats.hip): caller-made triples against the NumPy statement of
tests/content_stats_ref.py -- totals, histogram and locations per target, every number exact.

The kernel works on tiles of TILE = 2048 triples (a workgroup of 4 waves, each wave 512 contiguous triples in steps of 64); a run
that crosses a tile's end is followed by the tile's first wave; bins 1..4 are counted another way than the larger ones; targets are
summed over stretches of equal neighbours inside 64 triples."""
import importlib

import numpy as np
import pytest
import torch

import content_stats_ref as ref

pytestmark = pytest.mark.gpu
TILE = 2048          # CS_TILE of csrc/mcq_content_stats.hip
NT = 1000            # targets of the handle where the case does not say


def _eng():
    return importlib.import_module("metacache-mpi_amd.engine")


def _feat(lengths):
    lengths = np.asarray(lengths, np.int64)
    ids = (np.arange(len(lengths), dtype=np.uint64) * np.uint64(2654435761) + np.uint64(12345)) % np.uint64(0xFFFFFFFF)   # distinct: neighbours differ
    return np.repeat(ids.astype(np.uint32), lengths)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.uint32).view(np.int32).copy()).to(torch.device("cuda", 0))


def _add(cs, feat, tgt, how):
    """how: "host" = numpy arrays, "device" = device tensors, "offset" = device tensors that begin one element into their allocation"""
    if how == "host":
        cs.add(feat, tgt)
    elif how == "device":
        cs.add(_dev(feat), _dev(tgt), _dev(np.zeros(len(feat), np.uint32)))
    else:
        f, t = _dev(np.concatenate([[feat[0] if len(feat) else 0], feat])), _dev(np.concatenate([[NT + 5], tgt]))      # (the element in front: an equal feature, a bad target)
        cs.add(f[1:], t[1:])


def _check(feat, tgt, n_targets=NT, how="device"):
    cs = _eng().ContentStats(n_targets)
    _add(cs, feat, tgt, how)
    got, want = cs.totals(), ref.totals(feat)
    assert {k: v for k, v in got.items() if k != "hist"} == {k: int(v) for k, v in want.items() if k != "hist"}
    assert np.array_equal(got["hist"], want["hist"])
    assert np.array_equal(cs.target_locations(), ref.target_locations(tgt, n_targets))
    cs.close()
    return got


def _targets(lengths, mode, seed, n_targets=NT):
    """targets of every run: "blocks" = sorted blocks of equal targets inside each run (build order), "random", "equal" = one target"""
    rng = np.random.default_rng(seed)
    n = int(np.sum(lengths))
    if mode == "equal":
        return np.full(n, 7 % n_targets, np.uint32)
    t = rng.integers(0, n_targets, n, dtype=np.uint32)
    if mode == "blocks":
        start = np.concatenate([[0], np.cumsum(lengths)])
        for a, b in zip(start[:-1], start[1:]):
            t[a:b] = np.sort(rng.integers(0, min(n_targets, 6), b - a, dtype=np.uint32) * np.uint32(max(1, n_targets // 6 - 1)))
    return t


HOW = ["host", "device", "offset"]


@pytest.mark.parametrize("how", HOW)
def test_no_triples_and_one_triple(how):
    e = np.zeros(0, np.uint32)
    got = _check(e, e, how=how)
    assert got["n_buckets"] == 0 and got["max_size"] == 0 and got["hist"].sum() == 0
    got = _check(np.array([42], np.uint32), np.array([NT - 1], np.uint32), how=how)
    assert (got["n_buckets"], got["n_locations"], got["sum2"], got["sum3"], got["max_size"]) == (1, 1, 1, 1, 1)


@pytest.mark.parametrize("how", HOW)
def test_all_singletons_over_two_tiles_and_three(how):
    lengths = [1] * (2 * TILE + 3)
    got = _check(_feat(lengths), _targets(lengths, "random", 1), how=how)
    assert got["hist"][1] == 2 * TILE + 3


@pytest.mark.parametrize("how", ["host", "device"])
@pytest.mark.parametrize("length", [TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_one_run(length, how):
    got = _check(_feat([length]), _targets([length], "blocks", 2), how=how)
    assert got["n_buckets"] == 1 and got["max_size"] == length and got["hist"][255] == 1 and got["sum3"] == length ** 3


def test_runs_that_end_on_a_tile_edge():
    for lengths in ([TILE], [TILE, TILE], [TILE - 5, 5, 3, TILE - 3], [1000, 1048, 2048, 1], [64] * 32 + [512] * 4 + [1]):
        _check(_feat(lengths), _targets(lengths, "blocks", 3))


def test_a_run_over_three_tiles_with_short_runs_around_it():
    lengths = [1, 2, 3, 1, 100, 3 * TILE + 77, 1, 2, 254, 1]
    got = _check(_feat(lengths), _targets(lengths, "blocks", 4))
    assert got["max_size"] == 3 * TILE + 77 and got["n_buckets"] == len(lengths)


def test_sizes_around_the_histogram_clamp():
    lengths = [254, 255, 256, 300, 4, 5]
    got = _check(_feat(lengths), _targets(lengths, "random", 5))
    assert got["hist"][254] == 1 and got["hist"][255] == 3 and got["hist"][4] == 1 and got["hist"][5] == 1 and got["max_size"] == 300


def test_equal_features_in_two_runs_that_do_not_touch_are_two_buckets():
    feat = np.array([7, 7, 7, 9, 7, 7], np.uint32)
    got = _check(feat, np.zeros(6, np.uint32))
    assert got["n_buckets"] == 3 and got["hist"][3] == 1 and got["hist"][2] == 1 and got["hist"][1] == 1


@pytest.mark.parametrize("how", HOW)
@pytest.mark.parametrize("mode", ["blocks", "random", "equal"])
def test_random_run_lengths_over_five_tiles(mode, how):
    rng = np.random.default_rng(6)
    lengths = []
    while sum(lengths) < 5 * TILE - 300:
        lengths.append(int(rng.integers(1, 255)))
    _check(_feat(lengths), _targets(lengths, mode, 7), how=how)


def test_one_target_and_the_largest_valid_target():
    lengths = [3, 1, 70, 2, 200, 1]
    _check(_feat(lengths), np.zeros(sum(lengths), np.uint32), n_targets=1)
    t = _targets(lengths, "random", 8)
    t[[0, 5, 63, 64, 130, -1]] = NT - 1
    _check(_feat(lengths), t)


@pytest.mark.parametrize("how", ["host", "device"])
def test_a_target_out_of_range_is_refused_and_changes_nothing(how):
    eng = _eng()
    lengths = [3, 1, 70, 2, 200, 1, 2 * TILE]
    feat, tgt = _feat(lengths), _targets(lengths, "blocks", 9)
    cs = eng.ContentStats(NT)
    _add(cs, feat, tgt, how)
    before, counts = cs.totals(), cs.target_locations()
    bad = tgt.copy()
    bad[[150, TILE + 9]] = [NT, 0xFFFFFFFF]
    with pytest.raises(eng.McqError) as e:
        _add(cs, feat, bad, how)
    assert e.value.code == eng.MCQ_E_ARG and "triple 150 " in str(e.value) and "target %d" % NT in str(e.value)
    after = cs.totals()
    assert ref.same_totals(before, after) and np.array_equal(cs.target_locations(), counts)
    _add(cs, feat, tgt, how)                                # (and the handle goes on working)
    assert ref.same_totals(cs.totals(), ref.add_totals(ref.totals(feat), ref.totals(feat)))
    assert np.array_equal(cs.target_locations(), 2 * counts)
    cs.close()


def test_one_chunk_equals_the_chunks_cut_at_every_run_boundary():
    rng = np.random.default_rng(10)
    lengths = [int(x) for x in rng.integers(1, 120, 200)]
    while sum(lengths) < 3 * TILE - 50:
        lengths.append(int(rng.integers(1, 120)))
    feat, tgt = _feat(lengths), _targets(lengths, "blocks", 11)
    whole = _check(feat, tgt)
    cs = _eng().ContentStats(NT)
    df, dt = _dev(feat), _dev(tgt)
    start = np.concatenate([[0], np.cumsum(lengths)])
    for a, b in zip(start[:-1], start[1:]):
        cs.add(df[a:b], dt[a:b])
    assert ref.same_totals(cs.totals(), whole) and np.array_equal(cs.target_locations(), ref.target_locations(tgt, NT))
    cs.close()


def test_reset_between_two_inputs_keeps_the_target_counts():
    la, lb = [5, 1, 300, 2], [1, 1, 4, TILE + 1, 9]
    fa, ta, fb, tb = _feat(la), _targets(la, "random", 12), _feat(lb), _targets(lb, "blocks", 13)
    cs = _eng().ContentStats(NT)
    cs.add(fa, ta)
    assert ref.same_totals(cs.totals(), ref.totals(fa))
    cs.reset()
    assert cs.totals()["n_buckets"] == 0 and cs.totals()["hist"].sum() == 0
    cs.add(fb, tb)
    assert ref.same_totals(cs.totals(), ref.totals(fb))
    assert np.array_equal(cs.target_locations(), ref.target_locations(np.concatenate([ta, tb]), NT))
    cs.close()


def test_two_handles_alive_at_once():
    la, lb = [5, 1, 300, 2, TILE], [1, 1, 4, 9]
    fa, ta, fb, tb = _feat(la), _targets(la, "random", 14, 3), _feat(lb), _targets(lb, "random", 15, 50)
    a, b = _eng().ContentStats(3), _eng().ContentStats(50)
    a.add(fa, ta); b.add(_dev(fb), _dev(tb)); a.add(_dev(fb), _dev(tb % 3))
    assert ref.same_totals(b.totals(), ref.totals(fb)) and np.array_equal(b.target_locations(), ref.target_locations(tb, 50))
    assert ref.same_totals(a.totals(), ref.add_totals(ref.totals(fa), ref.totals(fb)))
    assert np.array_equal(a.target_locations(), ref.target_locations(np.concatenate([ta, tb % 3]), 3))
    a.close(); b.close()


def test_bad_arguments():
    eng = _eng()
    with pytest.raises(eng.McqError) as e:
        eng.ContentStats(0)
    assert e.value.code == eng.MCQ_E_ARG
    L = eng.lib()
    assert L.mcq_content_stats_add(None, None, None, None, 0, 0) == eng.MCQ_E_ARG
    cs = eng.ContentStats(4)
    assert L.mcq_content_stats_add(cs.h, None, None, None, 3, 0) == eng.MCQ_E_ARG
    cs.close()
