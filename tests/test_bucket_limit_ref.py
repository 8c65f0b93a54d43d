"""The NumPy statement of the query-time bucket rules (tests/bucket_limit_ref.py) on hand-written cases, and the mapping of
`-max-locations-per-feature N [-remove-overpopulated-features]` to the rule on the reference's quirk table -- for the NumPy
statement and for mcq_bucket_rule of include/mcq_open.hpp (compiled into a small program: it is header-only host code)."""
import os
import subprocess

import numpy as np
import pytest

import bucket_limit_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _chunk(lengths):
    """runs of the given lengths with distinct features; tgt counts the run, win the position in it"""
    feat = np.repeat(np.arange(len(lengths), dtype=np.uint32) * 7 + 3, lengths)
    tgt = np.repeat(np.arange(len(lengths), dtype=np.uint32), lengths)
    win = np.concatenate([np.arange(l, dtype=np.uint32) for l in lengths]) if len(lengths) else np.zeros(0, np.uint32)
    return feat, tgt, win


def test_shrink_keeps_the_first_of_every_long_bucket():
    f, t, w = _chunk([1, 3, 2, 5])
    of, ot, ow, shrunk, removed = ref.bucket_limit(f, t, w, keep_first=2)
    assert ot.tolist() == [0, 1, 1, 2, 2, 3, 3] and ow.tolist() == [0, 0, 1, 0, 1, 0, 1]
    assert of.tolist() == [3, 10, 10, 17, 17, 24, 24]
    assert (shrunk, removed) == (2, 0)


def test_removal_drops_whole_buckets_above_the_threshold():
    f, t, w = _chunk([1, 3, 2, 5])
    of, ot, ow, shrunk, removed = ref.bucket_limit(f, t, w, remove_above=2)
    assert ot.tolist() == [0, 2, 2] and ow.tolist() == [0, 0, 1] and (shrunk, removed) == (0, 2)


def test_removal_comes_first_then_the_shrink():
    f, t, w = _chunk([4, 2, 6, 1])
    of, ot, ow, shrunk, removed = ref.bucket_limit(f, t, w, keep_first=1, remove_above=4)
    assert ot.tolist() == [0, 1, 3] and ow.tolist() == [0, 0, 0] and (shrunk, removed) == (2, 1)    # the bucket of 6 goes, 4 and 2 are cut


def test_no_rule_and_no_triples():
    f, t, w = _chunk([2, 2])
    of, ot, ow, shrunk, removed = ref.bucket_limit(f, t, w)
    assert np.array_equal(of, f) and np.array_equal(ow, w) and (shrunk, removed) == (0, 0)
    e = np.zeros(0, np.uint32)
    of, ot, ow, shrunk, removed = ref.bucket_limit(e, e, e, keep_first=3, remove_above=2)
    assert len(of) == 0 and (shrunk, removed) == (0, 0)


def test_equal_features_apart_are_two_buckets():
    feat = np.array([5, 5, 5, 9, 5, 5, 5], np.uint32)          # (never in a real chunk; the rule is on maximal runs)
    z = np.arange(7, dtype=np.uint32)
    of, ot, ow, shrunk, removed = ref.bucket_limit(feat, z, z, keep_first=2)
    assert ow.tolist() == [0, 1, 3, 4, 5] and shrunk == 2


# (N, removal) -> (keep_first, remove_above), by hand from src/mode_query.cpp:354-377 and src/sketch_database.h:356-368, for a
# database limit of 254 and of 100.  The setter takes N as an 8-bit value: -1 -> 255 and 255, 254 mean "the largest" (no
# shrink), 0 -> 1, 300 -> 44.  The removal threshold is N - 1, 253 where that is negative or above 253, at most limit - 1, and
# used only when positive.
QUIRKS = {
    (-1, False): ((0, 0), (0, 0)),
    (0, False): ((0, 0), (0, 0)),
    (1, False): ((0, 0), (0, 0)),                  # "a value of 1 or less is ignored"
    (2, False): ((2, 0), (2, 0)),
    (254, False): ((0, 0), (0, 0)),
    (255, False): ((0, 0), (0, 0)),
    (300, False): ((44, 0), (44, 0)),
    (-1, True): ((0, 253), (0, 99)),
    (0, True): ((1, 253), (1, 99)),                # threshold from -1 -> 253; the setter makes 0 a 1
    (1, True): ((1, 0), (1, 0)),                   # threshold 0 is not applied: nothing removed, every bucket cut to one
    (2, True): ((2, 1), (2, 1)),
    (254, True): ((0, 253), (0, 99)),
    (255, True): ((0, 253), (0, 99)),
    (300, True): ((44, 253), (44, 99)),
}


@pytest.mark.parametrize("n,remove", sorted(QUIRKS))
def test_option_to_rule_mapping_on_the_quirk_table(n, remove):
    assert ref.bucket_rule(n, remove, 254) == QUIRKS[(n, remove)][0]
    assert ref.bucket_rule(n, remove, 100) == QUIRKS[(n, remove)][1]


def test_the_headers_mapping_gives_the_same_table(tmp_path):
    src = tmp_path / "rule.cpp"
    src.write_text('#include "mcq_open.hpp"\n#include <cstdio>\n'
                   'int main() { const int ns[7] = {-1, 0, 1, 2, 254, 255, 300}; const unsigned lim[2] = {254, 100};\n'
                   '  for (int n : ns) for (int r = 0; r < 2; ++r) for (unsigned l : lim) { uint32_t k, a; mcq_bucket_rule(n, r != 0, l, &k, &a);\n'
                   '    std::printf("%d %d %u %u %u\\n", n, r, l, k, a); }\n  return 0; }\n')
    exe = tmp_path / "rule"
    subprocess.check_call(["g++", "-std=c++14", "-pthread", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    rows = [tuple(int(x) for x in l.split()) for l in subprocess.check_output([str(exe)], text=True).split("\n") if l]
    assert len(rows) == 28
    for n, r, lim, k, a in rows:
        assert (k, a) == QUIRKS[(n, bool(r))][0 if lim == 254 else 1], (n, r, lim)
