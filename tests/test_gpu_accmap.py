"""mcq_accmap_* on the GPU (engine.AccMap) against the Python restatement of the reference's parser (tests/taxmap_ref.py) on
crafted texts of 30-400 lines and 6-40 names: every rule by which a line names a target, the first-line rule across chunks and
files, and the strict form -- a chunk that violates it is reported and changes nothing."""
import importlib
import random

import numpy as np
import pytest

import taxmap_ref as ref

pytestmark = pytest.mark.gpu
TILE = 4096


@pytest.fixture(scope="module")
def eng():
    import torch
    torch.zeros(1, device="cuda")            # (torch brings its GPU runtime up before the library makes its first call, as in the other tests)
    eng = importlib.import_module("metacache-mpi_amd.engine")
    eng.lib()
    return eng


def _dev(text, offset=0):
    """the text in device memory, `offset` bytes behind a 16-B aligned address: (tensor that owns it, pointer, length)"""
    import torch
    buf = torch.frombuffer(bytearray(b"\0" * offset + text + b"\0"), dtype=torch.uint8).cuda()
    return buf, buf.data_ptr() + offset, len(text)


def _feed(m, text, ordinal=0, line_no=0, offset=0):
    buf, ptr, n = _dev(text, offset)
    return m.chunk(ptr, n, ordinal, line_no)


def _gpu(eng, names, unranked, chunks):
    """chunks: [(text, ordinal, first line number)] in feeding order -> (all strict, parent list, found list)"""
    m = eng.AccMap(names, unranked)
    strict = [_feed(m, *c) for c in chunks]
    parent, found = m.finish()
    m.close()
    return all(strict), [int(p) for p in parent], [bool(f) for f in found]


def _want(names, unranked, files):
    """files: the texts in ordinal order (no header lines) -> (parent list, found list) by the restatement"""
    u, p = [bool(x) for x in unranked], [0] * len(names)
    N = ref.Names(names)
    for text in files:
        ref.accmap(text, N, u, p, skip_first_line=False)
    found = [bool(a) and not b for a, b in zip(unranked, u)]
    return [x if f else 0 for x, f in zip(p, found)], found


def _line(acc, accver, taxid, gi, end=b"\n"):
    return b"\t".join([acc, accver, str(taxid).encode(), gi]) + end


def crafted(seed, n_names, n_lines, long_fields=False):
    """names of every kind and lines that name them in every way, several times with different taxids, among lines that name
    nothing; about a third of the targets are ranked beforehand"""
    rng = random.Random(seed)
    names = []
    for i in range(n_names):
        kind = i % 4
        names.append([b"NC_%06d.%d" % (i * 7 + 1, 1 + i % 3), b"%d" % (5550000 + i), b"CP%05d" % i, b"scaffold_%d.1|x" % i][kind])
    unranked = [rng.random() < 0.7 for _ in names]
    lines = []
    for _ in range(n_lines):
        t = rng.randrange(n_names)
        nm, how = names[t], rng.randrange(6)
        tax = rng.choice([0, 1, 9, 562, 10 ** 18, 9999999999999999999, rng.randrange(1, 10 ** 7)])
        stem = nm.split(b".")[0]
        pad = b"x" * rng.randrange(0, 700) if long_fields and rng.random() < 0.1 else b""
        if how == 0:
            lines.append(_line(stem, nm, tax, b"%d" % rng.randrange(10 ** 8, 10 ** 9)))                 # by accver
        elif how == 1:
            lines.append(_line(stem, stem + b".99", tax, b"1" + pad))                                   # by acc (or by nothing)
        elif how == 2:
            lines.append(_line(b"QQ%05d" % rng.randrange(10 ** 5), b"QQ.1" + pad, tax, nm))             # by gi
        elif how == 3:
            other = names[rng.randrange(n_names)]
            lines.append(_line(stem, other, tax, nm))                                                   # accver names another target
        elif how == 4:
            lines.append(_line(nm[:max(1, len(nm) - 2)], b"none.1", tax, b"7"))                         # acc: a proper prefix of the name
        else:
            lines.append(_line(b"ZZ%06d" % rng.randrange(10 ** 6), b"ZZ.%d" % rng.randrange(9), tax, b"%d" % rng.randrange(10 ** 6)))
    return names, unranked, lines


@pytest.mark.parametrize("seed,n_names,n_lines", [(1, 6, 30), (2, 17, 150), (3, 40, 400)])
def test_one_chunk_against_the_restatement(eng, seed, n_names, n_lines):
    """400 lines are about 12 KiB: three tiles and more, lines across every tile boundary"""
    names, unranked, lines = crafted(seed, n_names, n_lines)
    text = b"".join(lines)
    assert ref.is_strict(text) and (n_lines < 400 or len(text) > 2 * TILE)
    strict, parent, found = _gpu(eng, names, unranked, [(text, 0, 0)])
    assert strict and (parent, found) == _want(names, unranked, [text])
    assert sum(found) >= 2


def test_every_matching_rule_by_hand(eng):
    names = [b"NC_1.1", b"NC_10.1", b"NC_2.1", b"NC_3.1", b"NC_5.1", b"777", b"NC_7", b"NC_8.1", b"NC_9.1"]
    text = b"".join([_line(b"NC_1", b"NC_1.1", 11, b"901"),        # accver
                     _line(b"NC_5", b"NC_5.2", 55, b"905"),        # acc: NC_5.2 names nobody, NC_5.1 is the first name behind NC_5
                     _line(b"ZZ_9", b"ZZ_9.1", 99, b"777"),        # gi
                     _line(b"NC_3", b"NC_3.1", 0, b"903"),         # a taxid of 0 counts ...
                     _line(b"NC_3", b"NC_3.1", 33, b"903"),        # ... and the later line is ignored
                     _line(b"NC_2", b"NC_8.1", 22, b"902"),        # accver names the RANKED NC_8.1: no falling through to NC_2.1
                     _line(b"NC_7", b"NC_7.5", 70, b"1"),          # acc equal to a name: not found (and NC_8.1 does not begin with it)
                     _line(b"NC_9", b"NC_9.1", 9999999999999999999, b"2"),
                     _line(b"NC_1", b"NC_1.3", 12, b"901")])       # NC_1.1 again, through acc: it has its taxid
    unranked = [True] * 9
    unranked[7] = False
    strict, parent, found = _gpu(eng, names, unranked, [(text, 0, 0)])
    assert strict and (parent, found) == _want(names, unranked, [text])
    assert parent == [11, 0, 0, 0, 55, 99, 0, 0, 9999999999999999999 - 2 ** 64]
    assert found == [True, False, False, True, True, True, False, False, True]


def test_the_prefix_quirk_and_a_name_equal_to_acc(eng):
    line = _line(b"NC_1", b"NC_1.7", 5, b"1")
    for names, hit in (([b"NC_10.1", b"NC_2.1"], 0),                 # no NC_1.*: NC_1 finds NC_10.1
                       ([b"NC_10.1", b"NC_2.1", b"NC_1.2"], 2),      # with one, that one
                       ([b"NC_1", b"NC_2.1"], None),                 # a name equal to acc is not found through acc
                       ([b"NC_1", b"NC_1.1"], 1),                    # ... the next name is, if it begins with acc
                       ([b"NC_0.1"], None), ([b"NC_1.7"], 0)):
        strict, parent, found = _gpu(eng, names, [True] * len(names), [(line, 0, 0)])
        assert strict and (parent, found) == _want(names, [True] * len(names), [line])
        assert [t for t, f in enumerate(found) if f] == ([] if hit is None else [hit]), names


def test_lines_up_to_the_cap_across_tile_boundaries(eng):
    """fields of up to 700 bytes; a line of exactly MCQ_ACCMAP_MAX_LINE bytes that starts 6 bytes before a tile boundary is strict
    and names its target, one byte more is not strict; the same text 1, 5 and 15 bytes off a 16-byte boundary"""
    names, unranked, lines = crafted(4, 20, 120, long_fields=True)
    pieces = [b"".join(lines)]
    need = (TILE - 6 - len(pieces[0])) % TILE + TILE                # filler lines up to 6 bytes before a tile boundary
    while need:
        n = 500 if need >= 1008 else need
        pieces.append(_line(b"A", b"B", 1, b"C" * (n - 7)))
        need -= n
    stub = _line(b"NC_000001", names[0], 424242, b"")
    long_ok = stub[:-1] + b"g" * (eng.MCQ_ACCMAP_MAX_LINE - len(stub)) + b"\n"
    text = b"".join(pieces) + long_ok + b"".join(lines[:20])
    assert len(long_ok) == eng.MCQ_ACCMAP_MAX_LINE and ref.is_strict(text) and len(b"".join(pieces)) % TILE == TILE - 6
    unranked = [True] * len(names)
    want = _want(names, unranked, [text])
    for offset in (0, 1, 5, 15):
        m = eng.AccMap(names, unranked)
        assert _feed(m, text, offset=offset)
        parent, found = m.finish()
        assert ([int(p) for p in parent], [bool(f) for f in found]) == want, offset
        m.close()
    too_long = text.replace(long_ok, long_ok[:-1] + b"g\n")
    assert not ref.is_strict(too_long)
    strict, parent, found = _gpu(eng, names, unranked, [(too_long, 0, 0)])
    assert not strict and not any(found)


def test_chunks_cut_at_every_line_boundary_give_what_one_chunk_gives(eng):
    names, unranked, lines = crafted(5, 24, 260)
    text = b"".join(lines)
    assert 2 * TILE < len(text) <= 3 * TILE + 2048
    one = _gpu(eng, names, unranked, [(text, 0, 0)])
    assert one[0] and one[1:] == _want(names, unranked, [text])
    cut = 0
    for line in lines[:-1]:
        cut += len(line)
        assert _gpu(eng, names, unranked, [(text[:cut], 0, 0), (text[cut:], 0, cut)]) == one, cut      # (line numbers: byte offsets)


def test_the_first_line_wins_across_chunks_and_files_fed_in_any_order(eng):
    """two files of two chunks each name the same targets with different taxids; whatever the feeding order, a target has the
    taxid of its first line in (ordinal, line number) order"""
    names, unranked, lines = crafted(6, 12, 240)
    a, b = b"".join(lines[:120]), b"".join(lines[120:])
    ca, cb = len(b"".join(lines[:50])), len(b"".join(lines[120:200]))
    chunks = [(a[:ca], 0, 0), (a[ca:], 0, 50), (b[:cb], 1, 0), (b[cb:], 1, 80)]
    want = _want(names, unranked, [a, b])
    assert want != _want(names, unranked, [b, a])                   # (the order of the files matters for this text)
    for order in ([0, 1, 2, 3], [3, 2, 1, 0], [2, 0, 3, 1], [1, 3, 0, 2]):
        strict, parent, found = _gpu(eng, names, unranked, [chunks[i] for i in order])
        assert strict and (parent, found) == want, order


BAD = {
    "an_empty_line": b"\n",
    "three_fields": b"A\tA.1\t5\n",
    "five_fields": b"A\tA.1\t5\t6\t7\n",
    "an_empty_first_field": b"\tA.1\t5\t6\n",
    "an_empty_second_field": b"A\t\t5\t6\n",
    "an_empty_taxid": b"A\tA.1\t\t6\n",
    "an_empty_last_field": b"A\tA.1\t5\t\n",
    "an_empty_last_field_before_cr": b"A\tA.1\t5\t\r\n",
    "a_space_in_a_field": b"A\tA .1\t5\t6\n",
    "spaces_for_tabs": b"A A.1 5 6\n",
    "a_vertical_tab": b"A\tA\v.1\t5\t6\n",
    "a_form_feed": b"A\tA.1\t5\t6\f\n",
    "a_cr_inside_the_line": b"A\tA.1\r\t5\t6\n",
    "two_crs": b"A\tA.1\t5\t6\r\r\n",
    "a_taxid_with_a_letter": b"A\tA.1\t5x\t6\n",
    "a_taxid_with_a_sign": b"A\tA.1\t+5\t6\n",
    "a_taxid_of_twenty_digits": b"A\tA.1\t12345678901234567890\t6\n",
    "a_line_beyond_the_cap": b"A\tA.1\t5\t" + b"6" * 1100 + b"\n",
}


@pytest.mark.parametrize("what", sorted(BAD))
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_a_chunk_that_is_not_strict_is_reported_and_changes_nothing(eng, what, where):
    names, unranked, lines = crafted(7, 16, 90)
    good1, good2 = b"".join(lines[:30]), b"".join(lines[30:60])
    at = {"first": 0, "middle": 15, "last": 30}[where]
    bad = b"".join(lines[60:60 + at]) + BAD[what] + b"".join(lines[60 + at:90])
    assert ref.is_strict(good1) and ref.is_strict(good2) and not ref.is_strict(bad)
    m = eng.AccMap(names, unranked)
    assert _feed(m, good1, 0, 0)
    before = m.finish()
    assert not _feed(m, bad, 0, 1000)
    after = m.finish()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert _feed(m, good2, 0, 2000)                                  # the handle goes on
    parent, found = m.finish()
    assert ([int(p) for p in parent], [bool(f) for f in found]) == _want(names, unranked, [good1 + good2])
    m.close()


def test_crlf_and_a_last_line_without_newline(eng):
    names, unranked, lines = crafted(8, 10, 60)
    text = b"".join(lines)
    crlf = text.replace(b"\n", b"\r\n")
    want = _want(names, unranked, [text])
    assert ref.is_strict(crlf) and _want(names, unranked, [crlf]) == want
    strict, parent, found = _gpu(eng, names, unranked, [(crlf, 0, 0)])
    assert strict and (parent, found) == want
    # the last line without its '\n' (with and without a '\r'): not strict -- the caller ends the file's last line himself
    for cut in (text[:-1], crlf[:-1], crlf[:-2]):
        assert not ref.is_strict(cut)
        m = eng.AccMap(names, unranked)
        assert not _feed(m, cut) and not m.finish()[1].any()
        assert _feed(m, cut + b"\n")
        parent, found = m.finish()
        assert ([int(p) for p in parent], [bool(f) for f in found]) == want
        m.close()
    m = eng.AccMap(names, unranked)
    assert m.chunk(0, 0) and not m.finish()[1].any()                 # an empty chunk is strict
    m.close()


def test_arguments_are_checked(eng):
    with pytest.raises(eng.McqError):
        eng.AccMap([b"b", b"a"], [1, 1]).chunk(0, 1 << 32)
    m = eng.AccMap([b"a"], [1])
    buf, ptr, n = _dev(_line(b"a", b"a", 1, b"a"))
    for ordinal, line_no in ((1 << 23, 0), (0, 1 << 40)):
        with pytest.raises(eng.McqError):
            m.chunk(ptr, n, ordinal, line_no)
    assert m.chunk(ptr, n, (1 << 23) - 1, (1 << 40) - 1 - n - 1) and m.finish()[1].all()
    blob, off, tgt = eng.sorted_names([b"b", b"a", b"b"])
    assert (blob, list(off), list(tgt)) == (b"ab", [0, 1, 2], [1, 0])
