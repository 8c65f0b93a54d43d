"""mcq_accmap_create_rule on the GPU (engine.AccMap(..., rule=)) against the Python restatement of annotate's map
(tests/annotate_ref.py: accmap_rule) on crafted texts of 30-400 lines and 6-40 names: under MCQ_ACCMAP_RULE_ACC / _ACCVER / _GI a
strict line names the name that EQUALS its first / second / fourth field and nothing else; the strict form, the first-line rule
across chunks and files, a taxid of 0 and the untouched handle after a chunk that is not strict are what they are under the default
rule (tests/test_gpu_accmap.py)."""
import importlib
import random

import numpy as np
import pytest

import annotate_ref as ar
import taxmap_ref as tr
from test_gpu_accmap import TILE, _dev, _feed, _line

pytestmark = pytest.mark.gpu
RULES = [ar.ACC, ar.ACCVER, ar.GI]


@pytest.fixture(scope="module")
def eng():
    import torch
    torch.zeros(1, device="cuda")            # (torch brings its GPU runtime up before the library makes its first call, as in the other tests)
    eng = importlib.import_module("metacache-mpi_amd.engine")
    eng.lib()
    assert (eng.MCQ_ACCMAP_RULE_ACC, eng.MCQ_ACCMAP_RULE_ACCVER, eng.MCQ_ACCMAP_RULE_GI) == (ar.ACC, ar.ACCVER, ar.GI)
    return eng


def _gpu(eng, names, unranked, chunks, rule, offset=0):
    """chunks: [(text, ordinal, first line number)] in feeding order -> (all strict, parent list, found list)"""
    m = eng.AccMap(names, unranked, rule=rule)
    strict = [_feed(m, *c, offset=offset) for c in chunks]
    parent, found = m.finish()
    m.close()
    return all(strict), [int(p) for p in parent], [bool(f) for f in found]


def _want(names, unranked, files, rule):
    """files: the texts in ordinal order (no first lines to pass over) -> (parent list, found list) by the restatement"""
    u, p = [bool(x) for x in unranked], [0] * len(names)
    for text in files:
        ar.accmap_rule(text, names, u, p, rule, skip_first_line=False)
    found = [bool(a) and not b for a, b in zip(unranked, u)]
    return [x if f else 0 for x, f in zip(p, found)], found


def crafted(seed, n_names, n_lines):
    """names that look like each of the three columns, and lines that hold them in every column -- the right one, a wrong one, as a
    proper prefix, beside the name of another target --, several times with different taxids, among lines that name nothing"""
    rng = random.Random(seed)
    names = [[b"NC_%06d" % (i * 7 + 1), b"NC_%06d.%d" % (i * 7 + 1, 1 + i % 3), b"%d" % (5550000 + i)][i % 3] for i in range(n_names)]
    unranked = [rng.random() < 0.8 for _ in names]
    lines = []
    for _ in range(n_lines):
        nm, other = names[rng.randrange(n_names)], names[rng.randrange(n_names)]
        tax = rng.choice([0, 1, 9, 562, 10 ** 18, 9999999999999999999, rng.randrange(1, 10 ** 7)])
        none = [b"ZZ%06d" % rng.randrange(10 ** 6), b"ZZ%06d.1" % rng.randrange(10 ** 6), b"%d" % rng.randrange(10 ** 8, 10 ** 9)]
        how = rng.randrange(7)
        if how < 3:
            cols = list(none)
            cols[how] = nm                                                   # the name in one column
        elif how == 3:
            cols = [nm, other, nm]                                           # names in all three
        elif how == 4:
            cols = [nm[:-1], nm + b"x", b"1" + nm]                           # a proper prefix, a longer one, another number
        elif how == 5:
            cols = [other, none[1], nm]
        else:
            cols = none
        lines.append(_line(cols[0], cols[1], tax, cols[2]))
    return names, unranked, lines


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("seed,n_names,n_lines", [(1, 6, 30), (2, 17, 150), (3, 40, 400)])
def test_one_chunk_against_the_restatement(eng, seed, n_names, n_lines, rule):
    names, unranked, lines = crafted(seed, n_names, n_lines)
    text = b"".join(lines)
    assert tr.is_strict(text) and (n_lines < 400 or len(text) > 2 * TILE)
    strict, parent, found = _gpu(eng, names, unranked, [(text, 0, 0)], rule)
    want = _want(names, unranked, [text], rule)
    assert strict and (parent, found) == want
    assert sum(found) >= 2
    others = [_want(names, unranked, [text], r) for r in RULES if r != rule]
    assert n_lines < 150 or all(o != want for o in others)              # (the text tells the rules apart)


def test_equal_to_one_column_and_nothing_else(eng):
    """acc is a proper prefix of a name and gi equals another: the default rule finds the first through taxon_with_similar_name; under
    _ACCVER the line names nothing, under _ACC nothing (a prefix is not the name), under _GI the second"""
    names, line = [b"NC_10.1", b"777"], _line(b"NC_1", b"NC_1.7", 5, b"777")
    u = [True, True]
    m = eng.AccMap(names, u)                                                # the two-argument form: the default rule
    assert _feed(m, line)
    parent, found = m.finish()
    m.close()
    assert list(found) == [True, False] and int(parent[0]) == 5
    assert _gpu(eng, names, u, [(line, 0, 0)], eng.MCQ_ACCMAP_RULE_TARGETS) == (True, [5, 0], [True, False])
    assert _gpu(eng, names, u, [(line, 0, 0)], ar.ACCVER) == (True, [0, 0], [False, False])
    assert _gpu(eng, names, u, [(line, 0, 0)], ar.ACC) == (True, [0, 0], [False, False])
    assert _gpu(eng, names, u, [(line, 0, 0)], ar.GI) == (True, [0, 5], [False, True])
    for rule in RULES:
        assert _gpu(eng, names, u, [(line, 0, 0)], rule)[1:] == _want(names, u, [line], rule)
    # a ranked name stays what it is under every rule
    assert _gpu(eng, names, [True, False], [(line, 0, 0)], ar.GI) == (True, [0, 0], [False, False])
    with pytest.raises(eng.McqError):
        eng.AccMap(names, u, rule=4)


@pytest.mark.parametrize("rule", RULES)
def test_the_first_line_wins_across_chunks_and_files_fed_in_reverse(eng, rule):
    names, unranked, lines = crafted(6, 12, 240)
    a, b = b"".join(lines[:120]), b"".join(lines[120:])
    ca, cb = len(b"".join(lines[:50])), len(b"".join(lines[120:200]))
    chunks = [(a[:ca], 0, 0), (a[ca:], 0, ca), (b[:cb], 1, 0), (b[cb:], 1, cb)]
    want = _want(names, unranked, [a, b], rule)
    assert want != _want(names, unranked, [b, a], rule)                 # (the order of the files matters for this text)
    for order in ([0, 1, 2, 3], [3, 2, 1, 0], [2, 0, 3, 1]):
        strict, parent, found = _gpu(eng, names, unranked, [chunks[i] for i in order], rule)
        assert strict and (parent, found) == want, order


@pytest.mark.parametrize("rule", RULES)
def test_two_chunks_cut_at_every_line_boundary(eng, rule):
    names, unranked, lines = crafted(5, 8, 30)
    text = b"".join(lines)
    one = _gpu(eng, names, unranked, [(text, 0, 0)], rule)
    assert one[0] and one[1:] == _want(names, unranked, [text], rule) and sum(one[2]) >= 2
    cut = 0
    for line in lines[:-1]:
        cut += len(line)
        assert _gpu(eng, names, unranked, [(text[cut:], 0, cut), (text[:cut], 0, 0)], rule) == one, cut


@pytest.mark.parametrize("rule", RULES)
def test_tile_edge_line_cap_and_alignment(eng, rule):
    """a naming line that begins 6 bytes before the 4096-byte tile edge; a line of exactly MCQ_ACCMAP_MAX_LINE bytes that names a name;
    the text 1 to 15 bytes off 16-byte alignment; one byte more than the cap: not strict, the handle unchanged"""
    names, unranked, lines = crafted(4, 20, 60)
    unranked = [True] * len(names)
    col = {ar.ACC: 0, ar.ACCVER: 1, ar.GI: 2}[rule]
    base = _want(names, unranked, [b"".join(lines)], rule)[1]
    nm, nm2 = [n for n, f in zip(names, base) if not f][:2]                  # two names that only the lines below name

    def naming(name, tax, pad_to=0):
        cols = [b"QQ1", b"QQ1.1", b"12"]
        cols[col] = name
        other = 1 if col != 1 else 0                                          # the padding goes into a column that is not looked up
        line = _line(cols[0], cols[1], tax, cols[2])
        if pad_to:
            cols[other] = cols[other] + b"g" * (pad_to - len(line))
            line = _line(cols[0], cols[1], tax, cols[2])
        return line

    pieces = [b"".join(lines)]
    need = (TILE - 6 - len(pieces[0])) % TILE + TILE
    while need:
        n = 500 if need >= 1008 else need
        pieces.append(_line(b"A", b"B", 1, b"C" * (n - 7)))
        need -= n
    head = b"".join(pieces)
    straddle, long_ok = naming(nm, 424242), naming(nm2, 77, eng.MCQ_ACCMAP_MAX_LINE)
    text = head + straddle + long_ok + b"".join(lines[:20])
    assert len(head) % TILE == TILE - 6 and len(straddle) > 6 and len(long_ok) == eng.MCQ_ACCMAP_MAX_LINE and tr.is_strict(text)
    want = _want(names, unranked, [text], rule)
    assert want[0][names.index(nm)] == 424242 and want[0][names.index(nm2)] == 77
    for offset in range(16):
        assert _gpu(eng, names, unranked, [(text, 0, 0)], rule, offset=offset) == (True,) + want, offset
    too_long = text.replace(long_ok, naming(nm2, 77, eng.MCQ_ACCMAP_MAX_LINE + 1))
    assert not tr.is_strict(too_long)
    m = eng.AccMap(names, unranked, rule=rule)
    assert _feed(m, head + straddle, 0, 0)
    before = m.finish()
    assert not _feed(m, too_long, 0, 1 << 20)
    after = m.finish()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and before[1].sum() >= 1
    m.close()


@pytest.mark.parametrize("rule", RULES)
def test_crlf_and_a_taxid_of_zero_as_first_line(eng, rule):
    names, unranked, lines = crafted(8, 10, 60)
    text = b"".join(lines)
    crlf = text.replace(b"\n", b"\r\n")
    want = _want(names, unranked, [text], rule)
    assert tr.is_strict(crlf) and _want(names, unranked, [crlf], rule) == want and sum(want[1]) >= 2
    assert _gpu(eng, names, unranked, [(crlf, 0, 0)], rule) == (True,) + want
    cols = [b"X", b"X.1", b"9"]
    cols[{ar.ACC: 0, ar.ACCVER: 1, ar.GI: 2}[rule]] = names[0]
    zero_first = _line(cols[0], cols[1], 0, cols[2]) + _line(cols[0], cols[1], 55, cols[2])
    strict, parent, found = _gpu(eng, names, [True] * len(names), [(zero_first, 0, 0)], rule)
    assert strict and found[0] and parent[0] == 0 and sum(found) == 1
    assert (parent, found) == _want(names, [True] * len(names), [zero_first], rule)
