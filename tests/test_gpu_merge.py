"""mcq_merge_* on the GPU (engine.Merge) against the Python restatement of the reference's merge mode (tests/merge_ref.py), on a
made-up taxonomy of 80 species with two subspecies and a strain, and on the `mini` database's taxonomy for the classification:
every rule of the insert with one line per case, lines at every position around a tile boundary and up to the length cap, chunks
cut at every line boundary, and the strict form -- a chunk that violates it is reported and changes nothing."""
import importlib
import os
import random

import numpy as np
import pytest

import merge_ref as ref

pytestmark = pytest.mark.gpu
TILE = 4096
R = ref.RANK
HERE = os.path.dirname(os.path.abspath(__file__))


def _taxa():
    """root 1 > domain 2 > phylum 10 > class 20 > order 30 > families 40, 41 > genera 100 .. 800 > species g + 1 .. g + 10; species 101
    has the subspecies 1011 and 1012, and 1011 a strain without rank, 1013"""
    t = [(1, 1, R["none"]), (2, 1, R["domain"]), (10, 2, R["phylum"]), (20, 10, R["class"]), (30, 20, R["order"]), (40, 30, R["family"]),
         (41, 30, R["family"])]
    for g in range(100, 900, 100):
        t.append((g, 40 if g <= 400 else 41, R["genus"]))
        t += [(g + s, g, R["species"]) for s in range(1, 11)]
    t += [(1011, 101, R["subspecies"]), (1012, 101, R["subspecies"]), (1013, 1011, R["none"])]
    return sorted(t)


T = ref.Tax(_taxa())
TABLE = (np.sort(np.array(T.ids, np.int64)), np.argsort(np.array(T.ids, np.int64)).astype(np.uint32))     # (the ids are distinct)
SPECIES = [i for i in T.ids if T.rank[T.index[i]] == R["species"]]


@pytest.fixture(scope="module")
def eng():
    import torch
    torch.zeros(1, device="cuda")            # (torch brings its GPU runtime up before the library makes its first call, as in the other tests)
    eng = importlib.import_module("metacache-mpi_amd.engine")
    eng.lib()
    assert (eng.MCQ_MERGE_MAX_LINE, eng.MCQ_MERGE_MAX_ITEMS) == (ref.MAX_LINE, ref.MAX_ITEMS)
    return eng


@pytest.fixture(scope="module")
def tax(eng):
    return eng.Taxonomy(T.lineage, T.rank)


def _dev(text, offset=0):
    """the text in device memory, `offset` bytes behind a 16-B aligned address: (tensor that owns it, pointer, length)"""
    import torch
    buf = torch.frombuffer(bytearray(b"\0" * offset + text + b"\0"), dtype=torch.uint8).cuda()
    return buf, buf.data_ptr() + offset, len(text)


def _feed(m, text, ordinal=0, chunk_offset=0, offset=0, column=2):
    buf, ptr, n = _dev(text, offset)
    return m.chunk(ptr, n, ordinal, chunk_offset, column)


def line(qid, items, header=None, tail=b"species:x\t|\n"):
    """`id | header | top_hits | ...` as mcq_query_cli -tophits -queryids writes it; items: [(taxid, hits)]"""
    header = b"read_%d/1" % qid if header is None else header
    return b"%d\t|\t%s\t|\t%s\t|\t%s" % (qid, header, b",".join(b"%d:%d" % it for it in items), tail)


def _state(m):
    n, pairs, unknown = m.lists()
    f, o, l = m.headers()
    return [x.tobytes() for x in (n, pairs, f, o, l)] + [unknown]


def _check(m, want, files=None):
    """the handle's lists, unknown count and (with the files' texts, in ordinal order) header tokens against a ref.Merged"""
    n, pairs, unknown = m.lists()
    wn, wp = want.as_arrays()
    assert np.array_equal(n, wn) and np.array_equal(pairs, wp) and unknown == want.unknown
    if files is not None:
        f, o, l = m.headers()
        got = [files[f[q]][int(o[q]):int(o[q]) + int(l[q])] for q in range(len(n))]
        assert got == want.headers


def _run(eng, tax, files, n_queries, max_cand=4, merge_below=R["species"]):
    """every file as one chunk, in order, on the GPU and through the restatement; returns the ids of each list for by-hand checks"""
    m = eng.Merge(tax, TABLE, n_queries, max_cand, merge_below)
    want = ref.Merged(T, n_queries, max_cand, merge_below)
    for k, text in enumerate(files):
        assert ref.is_strict(text, n_queries)
        assert _feed(m, text, k)
        want.read_results(text)
    _check(m, want, files)
    m.close()
    return [[(T.ids[t], h) for t, h in l] for l in want.lists], want.unknown


RULES = {
    "equal_hits_keep_the_earlier_entry": (4, [[(101, 7)], [(102, 7)]], [(101, 7), (102, 7)], 0),
    "a_tie_with_the_last_entry_of_a_full_list_is_dropped": (2, [[(101, 9), (102, 7)], [(201, 7)]], [(101, 9), (102, 7)], 0),
    "more_hits_than_the_last_entry_of_a_full_list_replace_it": (2, [[(101, 9), (102, 7)], [(201, 8)]], [(101, 9), (201, 8)], 0),
    "an_update_with_more_hits_moves_ahead_of_smaller_and_behind_equal": (4, [[(101, 9), (102, 7), (201, 5)], [(201, 9)]],
                                                                         [(101, 9), (201, 9), (102, 7)], 0),
    "an_update_with_fewer_hits_changes_nothing": (4, [[(101, 9), (102, 7)], [(102, 6)]], [(101, 9), (102, 7)], 0),
    "an_update_with_equal_hits_changes_nothing": (4, [[(101, 7), (102, 7)], [(102, 7)]], [(101, 7), (102, 7)], 0),
    "two_subspecies_rise_to_one_species": (4, [[(1011, 5), (1012, 8)]], [(101, 8)], 0),
    "a_strain_without_rank_rises_to_its_species": (4, [[(1013, 5)], [(101, 4)]], [(101, 5)], 0),
    "a_rank_above_lowest_is_kept": (4, [[(100, 6), (101, 6), (30, 2)]], [(100, 6), (101, 6), (30, 2)], 0),
    "an_unknown_taxid_is_skipped_and_counted": (4, [[(999, 9), (101, 3)], [(7, 1), (555555555555555555, 2)]], [(101, 3)], 3),
    "no_item": (4, [[]], [], 0),
    "one_item": (4, [[(301, 999999999)]], [(301, 999999999)], 0),
}


@pytest.mark.parametrize("rule", sorted(RULES))
def test_every_insert_rule_with_one_line_per_file(eng, tax, rule):
    max_cand, files, merged, unknown = RULES[rule]
    lists, n_unknown = _run(eng, tax, [line(1, items) for items in files], 1, max_cand)
    assert lists == [merged] and n_unknown == unknown


@pytest.mark.parametrize("max_cand", [1, 2, 4, 16])
def test_item_counts_around_the_list_capacity_and_up_to_the_cap(eng, tax, max_cand):
    """0, 1, max_cand, max_cand + 1 and MCQ_MERGE_MAX_ITEMS items in a line, ascending hits (every item goes to the front) and
    descending (the list fills and the rest is dropped), and one subspecies line among them"""
    rng = random.Random(max_cand)
    ids = [rng.sample(SPECIES, n) for n in (0, 1, max_cand, max_cand + 1, ref.MAX_ITEMS)]
    files = []
    for order in (1, -1):                                        # (the second file: the same taxa, every other one with one hit more)
        lines = []
        for q in range(5):
            lines.append(line(q + 1, [(t, 10 + i + (i % 2 if order < 0 else 0)) for i, t in enumerate(ids[q])][::order]))
        lines.append(line(6, [(1012, 3), (1011, 4), (1013, 4), (101, 2)]))
        files.append(b"".join(lines))
    lists, _ = _run(eng, tax, files, 6, max_cand)
    assert [len(l) for l in lists] == [0, 1, max_cand, max_cand, max_cand, 1] and lists[5] == [(101, 4)]


def test_the_taxon_is_kept_without_a_merge_rank(eng, tax):
    lists, _ = _run(eng, tax, [line(1, [(1011, 5), (1012, 8), (1013, 8)])], 1, 4, merge_below=0)
    assert lists == [[(1012, 8), (1013, 8), (1011, 5)]]


def _filler(n):
    """n bytes of comment lines (n >= 2)"""
    out = []
    while n:
        k = n if n <= 300 else 298
        out.append(b"#" + b"c" * (k - 2) + b"\n")
        n -= k
    return b"".join(out)


def test_a_line_beginning_at_each_of_the_last_bytes_of_a_tile_and_at_the_next_tile(eng, tax):
    m = eng.Merge(tax, TABLE, 9, 4)
    want = ref.Merged(T, 9, 4)
    files = []
    for k in range(9):                                           # the line begins k bytes before the second tile
        text = _filler(TILE - k) + line(k + 1, [(101 + k, 5 + k), (201, 3)]) + _filler(40)
        assert text[TILE - k - 1:TILE - k] == b"\n" and ref.is_strict(text, 9)
        assert _feed(m, text, k)
        want.read_results(text)
        files.append(text)
    _check(m, want, files)
    m.close()


@pytest.mark.parametrize("offset", [0, 1, 5, 15])
def test_lines_up_to_the_length_cap_across_a_tile_boundary_at_any_address(eng, tax, offset):
    """a line of exactly MCQ_MERGE_MAX_LINE bytes that begins 6 bytes before a tile boundary is strict and applied; one byte more is
    not strict; the text 0, 1, 5 and 15 bytes off a 16-byte boundary"""
    stub = line(2, [(101, 7), (1011, 9)], tail=b"")
    long_ok = stub + b"g" * (ref.MAX_LINE - len(stub) - 1) + b"\n"
    text = line(1, [(201, 4)]) + _filler(TILE - 6 - len(line(1, [(201, 4)]))) + long_ok + line(3, [(301, 2)])
    assert len(long_ok) == ref.MAX_LINE and text.index(long_ok) == TILE - 6 and ref.is_strict(text, 3)
    m = eng.Merge(tax, TABLE, 3, 4)
    want = ref.Merged(T, 3, 4)
    assert _feed(m, text, offset=offset)
    want.read_results(text)
    _check(m, want, [text])
    assert want.lists[1] == [[T.index[101], 9]]
    before = _state(m)
    too_long = text.replace(long_ok, long_ok[:-1] + b"g\n")
    assert not ref.is_strict(too_long, 3)
    assert not _feed(m, too_long, 1, offset=offset) and _state(m) == before
    m.close()


def test_a_last_line_without_lf_and_an_empty_chunk(eng, tax):
    text = line(1, [(101, 7)]) + line(2, [(102, 8)], tail=b"species:x")
    assert not text.endswith(b"\n") and ref.is_strict(text, 2)
    m = eng.Merge(tax, TABLE, 2, 2)
    want = ref.Merged(T, 2, 2)
    assert m.chunk(0, 0) and _feed(m, text)
    want.read_results(text)
    _check(m, want, [text])
    short = line(1, [(103, 9)]) + line(2, [(104, 9)])[:-len(b"species:x\t|\n")]      # ends behind the TAB of top_hits
    assert short.endswith(b"\t") and _feed(m, short, 1)
    want.read_results(short)
    _check(m, want, [text, short])
    m.close()


def crafted(seed, n_queries, comments=False, pad=0):
    """one results file: every query once, in order, 0-6 items each from a pool of 12 species, subspecies, a genus and unknown ids"""
    rng = random.Random(seed)
    pool = SPECIES[:10] + [201, 301, 1011, 1012, 1013, 100, 999, 31337]
    out = [b"# a comment in front\n"] if comments else []
    for q in range(1, n_queries + 1):
        items = [(t, rng.randrange(1, 12)) for t in rng.sample(pool, rng.randrange(0, 7))]
        items.sort(key=lambda it: -it[1])
        out.append(line(q, items, tail=b"genus:" + b"n" * rng.randrange(0, pad + 1) + b"\t|\n"))
        if comments and rng.random() < 0.1:
            out.append(b"#\n" if rng.random() < 0.5 else b"# between | the \t lines\n")
    if comments:
        out.append(b"# a comment behind\n# and one more")
    return out


FILES = [crafted(seed, 90, pad=120) for seed in (11, 12, 13)]


def test_three_files_cut_at_every_line_boundary_give_what_whole_files_give(eng, tax):
    texts = [b"".join(f) for f in FILES]
    assert all(len(t) > 2 * TILE - 1024 for t in texts)
    want = ref.Merged(T, 90, 4)
    for t in texts:
        want.read_results(t)
    changed = sum(1 for q in range(90) if all(want.lists[q] != one.lists[q] for one in _singles(texts)))
    assert changed >= 9                                          # (a merge that changes nothing pins nothing)
    for which in range(3):
        cut = 0
        for ln in FILES[which][:-1]:
            cut += len(ln)
            m = eng.Merge(tax, TABLE, 90, 4)
            for k, t in enumerate(texts):
                if k == which:
                    assert _feed(m, t[:cut], k, 0) and _feed(m, t[cut:], k, cut)
                else:
                    assert _feed(m, t, k)
            _check(m, want, texts)
            m.close()


def _singles(texts):
    out = []
    for t in texts:
        one = ref.Merged(T, 90, 4)
        one.read_results(t)
        out.append(one)
    return out


def test_the_golden_result_files_cut_at_every_line_boundary(eng):
    """the reference's three result files of tests/golden/merge over the `mini` taxonomy: one chunk per file gives what the
    restatement gives (which test_merge_ref.py holds against the reference's merged files), and so does every cut of one file"""
    from test_merge_ref import golden_results, T as M
    files = golden_results()
    table = (np.sort(np.array(M.ids, np.int64)), np.argsort(np.array(M.ids, np.int64)).astype(np.uint32))
    mtax = eng.Taxonomy(M.lineage, M.rank)
    want = ref.Merged(M, 293, 4)
    for body, col, n in files:
        want.read_results(body, col)
    texts = [f[0] for f in files]
    for which in range(3):
        cuts = [i + 1 for i, c in enumerate(texts[which][:-1]) if c == 10]
        for cut in [0] + cuts:
            m = eng.Merge(mtax, table, 293, 4)
            for k, t in enumerate(texts):
                if k == which and cut:
                    assert _feed(m, t[:cut], k, 0) and _feed(m, t[cut:], k, cut)
                else:
                    assert _feed(m, t, k)
            n, pairs, unknown = m.lists()
            wn, wp = want.as_arrays()
            assert np.array_equal(n, wn) and np.array_equal(pairs, wp) and unknown == 0, (which, cut)
            if not cut:
                f, o, l = m.headers()
                assert [texts[f[q]][int(o[q]):int(o[q]) + int(l[q])] for q in range(293)] == want.headers
            m.close()


def test_the_order_of_the_files_is_part_of_the_result(eng, tax):
    texts = [b"".join(f) for f in FILES]
    seen = set()
    for order in ([0, 1, 2], [2, 1, 0], [1, 2, 0]):
        m = eng.Merge(tax, TABLE, 90, 4)
        want = ref.Merged(T, 90, 4)
        for k, i in enumerate(order):
            assert _feed(m, texts[i], k)
            want.read_results(texts[i])
        _check(m, want, [texts[i] for i in order])
        seen.add(want.as_arrays()[1].tobytes())
        m.close()
    assert len(seen) > 1


def test_ids_out_of_order_inside_a_file_give_the_same_lists(eng, tax):
    want = ref.Merged(T, 90, 4)
    m = eng.Merge(tax, TABLE, 90, 4)
    for k, f in enumerate(FILES):
        want.read_results(b"".join(f))
        shuffled = list(f)
        random.Random(k).shuffle(shuffled)
        assert shuffled != f and _feed(m, b"".join(shuffled), k)
    n, pairs, unknown = m.lists()
    wn, wp = want.as_arrays()
    assert np.array_equal(n, wn) and np.array_equal(pairs, wp) and unknown == want.unknown
    m.close()


def test_comment_lines_in_front_between_and_behind(eng, tax):
    files = [b"".join(crafted(seed, 40, comments=True)) for seed in (21, 22)]
    assert all(f.count(b"\n#") >= 3 and f.startswith(b"#") and not f.endswith(b"\n") for f in files)
    _run(eng, tax, files, 40)


def test_a_layout_with_more_columns_in_front_of_top_hits(eng, tax):
    text = b"".join(b"%d\t|\tr%d\t|\tanything at\tall\t|\t\t|\t%d:5,201:5\t|\tx\n" % (q, q, 100 + q) for q in range(1, 6))
    m = eng.Merge(tax, TABLE, 5, 2)
    want = ref.Merged(T, 5, 2)
    assert ref.is_strict(text, 5, 4) and _feed(m, text, column=4)
    want.read_results(text, 4)
    _check(m, want, [text])
    assert all(len(l) == 2 for l in want.lists)
    m.close()


GOOD = line(7, [(101, 5), (102, 4)])
BAD = {
    "an_empty_line": b"\n",
    "no_id": b"\t|\tr\t|\t101:5\t|\tx\n",
    "an_id_of_zero": line(0, [(101, 5)]),
    "an_id_beyond_the_queries": line(31, [(101, 5)]),
    "an_id_with_a_sign": b"+" + GOOD,
    "an_id_with_a_letter": b"7x" + GOOD[1:],
    "an_id_of_nineteen_digits": b"000000000000000000" + GOOD,
    "a_blank_in_front_of_the_id": b" " + GOOD,
    "spaces_for_the_first_separator": GOOD.replace(b"7\t|\t", b"7 | ", 1),
    "no_tab_behind_the_first_bar": GOOD.replace(b"7\t|\t", b"7\t|", 1),
    "an_empty_header_column": line(7, [(101, 5)], header=b""),
    "a_header_that_begins_with_a_blank": line(7, [(101, 5)], header=b" r7"),
    "a_bar_in_the_header": line(7, [(101, 5)], header=b"q7 taxid|562"),
    "a_bar_at_the_end_of_the_header": line(7, [(101, 5)], header=b"q7|"),
    "a_header_column_without_its_separator": b"7\t|\tr7|\t101:5\t|\tx\n",
    "a_line_that_ends_in_the_header": b"7\t|\tr7\n",
    "no_tab_behind_the_bar_in_front_of_top_hits": b"7\t|\tr7\t|101:5\t|\tx\n",
    "an_item_that_is_a_name": b"7\t|\tr7\t|\tNC_000913.3:5\t|\tx\n",
    "an_item_without_hits": b"7\t|\tr7\t|\t101:\t|\tx\n",
    "an_item_without_colon": b"7\t|\tr7\t|\t101\t|\tx\n",
    "an_item_with_two_colons": b"7\t|\tr7\t|\t101:5:5\t|\tx\n",
    "a_negative_taxid": b"7\t|\tr7\t|\t-101:5\t|\tx\n",
    "a_taxid_of_nineteen_digits": b"7\t|\tr7\t|\t1234567890123456789:5\t|\tx\n",
    "hits_of_ten_digits": b"7\t|\tr7\t|\t101:4294967296\t|\tx\n",
    "hits_that_overflow": b"7\t|\tr7\t|\t101:99999999999999999999\t|\tx\n",
    "two_commas": b"7\t|\tr7\t|\t101:5,,102:4\t|\tx\n",
    "a_comma_at_the_end": b"7\t|\tr7\t|\t101:5,\t|\tx\n",
    "a_blank_behind_a_comma": b"7\t|\tr7\t|\t101:5, 102:4\t|\tx\n",
    "a_blank_in_front_of_the_items": b"7\t|\tr7\t|\t 101:5\t|\tx\n",
    "no_tab_behind_the_items": b"7\t|\tr7\t|\t101:5\n",
    "one_item_too_many": line(7, [(t, 3) for t in SPECIES[:ref.MAX_ITEMS + 1]]),
    "a_line_beyond_the_length_cap": line(7, [(101, 5)], tail=b"x" * ref.MAX_LINE + b"\n"),
    "an_id_twice": line(3, [(101, 5)]),
}


@pytest.mark.parametrize("what", sorted(BAD))
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_a_chunk_that_is_not_strict_is_reported_and_changes_nothing(eng, tax, what, where):
    lines = crafted(31, 6)
    good1, good2 = b"".join(lines), b"".join(crafted(32, 6))
    at = {"first": 0, "middle": 3, "last": 6}[where]
    bad = b"".join(lines[:at]) + BAD[what] + b"".join(lines[at:])
    assert ref.is_strict(good1, 30) and not ref.is_strict(bad, 30)
    m = eng.Merge(tax, TABLE, 30, 4)
    want = ref.Merged(T, 30, 4)
    assert _feed(m, good1, 0)
    want.read_results(good1)
    before = _state(m)
    assert not _feed(m, bad, 1)
    assert _state(m) == before                                   # byte for byte: counts, pairs, header references, the unknown count
    assert _feed(m, good2, 1)                                    # the handle goes on
    want.read_results(good2)
    _check(m, want, [good1, good2])
    m.close()


def test_parsed_lines_against_the_insert_alone(eng, tax):
    """mcq_merge_lines on caller-made lines: 300 queries in three calls (more than one workgroup), every id once per call"""
    rng = random.Random(5)
    pool = SPECIES[:14] + [1011, 1012, 1013, 100, 40, 999]
    n_q = 300
    m = eng.Merge(tax, TABLE, n_q, 3)
    want = [[] for _ in range(n_q)]
    unknown = 0
    for call in range(3):
        qs = rng.sample(range(n_q), 280)
        off, tid, hits = [0], [], []
        for q in qs:
            for t in rng.sample(pool, rng.randrange(0, 9)):
                h = rng.randrange(1, 9)
                tid.append(t); hits.append(h)
                if t in T.index:
                    ref.insert(want[q], T.index[t], h, T, 3, R["species"])
                else:
                    unknown += 1
            off.append(len(tid))
        m.lines(qs, off, tid, hits, header_off=[7 * q for q in qs], header_len=[call + 1] * len(qs), file_ordinal=call)
    n, pairs, n_unknown = m.lists()
    assert n_unknown == unknown
    for q in range(n_q):
        assert [list(map(int, p)) for p in pairs[q, :n[q]]] == want[q], q
    f, o, l = m.headers()
    assert all(l[q] == f[q] + 1 and o[q] == 7 * q for q in range(n_q) if l[q]) and (l > 0).sum() > 290
    before = _state(m)
    with pytest.raises(eng.McqError):                            # a query twice in one call: nothing is applied
        m.lines([1, 2, 1], [0, 1, 2, 3], [101, 102, 103], [50, 50, 50])
    with pytest.raises(eng.McqError):
        m.lines([n_q], [0, 1], [101], [50])
    assert _state(m) == before
    m.close()


def test_text_that_is_not_strict_through_the_host_parser_and_the_parsed_lines(eng, tax):
    """what a caller does with a chunk that is reported: mcq_merge_host, then mcq_merge_lines cut at repeated ids"""
    host = importlib.import_module("metacache-mpi_amd.host")
    loose = [b"".join(f).replace(b"\t|\t", b" |\t", 1) for f in FILES]           # a blank in front of the first bar of the text
    loose[1] = b"".join(FILES[1] + FILES[2][:40])                                   # ids that repeat inside one text
    loose[2] = b"\n" + b"".join(l.replace(b",", b", ", 1) for l in FILES[2])        # an empty line, a blank behind a comma
    m = eng.Merge(tax, TABLE, 90, 4)
    want = ref.Merged(T, 90, 4)
    for k, text in enumerate(loose):
        assert not ref.is_strict(text, 90)
        before = _state(m)
        assert not _feed(m, text, k) and _state(m) == before
        m.lines_cut(*host.merge_host(text, 90), file_ordinal=k)
        want.read_results(text)
    _check(m, want, loose)
    m.close()


def test_arguments_are_checked(eng, tax):
    for max_cand in (0, 17):
        with pytest.raises(eng.McqError):
            eng.Merge(tax, TABLE, 4, max_cand)
    with pytest.raises(eng.McqError):
        eng.Merge(tax, TABLE, 4, 2, merge_below_rank=21)
    m = eng.Merge(tax, TABLE, 4, 2)
    buf, ptr, n = _dev(line(1, [(101, 5)]))
    for column in (0, 1):
        with pytest.raises(eng.McqError):
            m.chunk(ptr, n, 0, 0, column)
    with pytest.raises(eng.McqError):
        m.chunk(ptr, 1 << 32)
    assert m.lists()[0].sum() == 0
    m.close()


def test_finish_classifies_as_the_host_library_does_at_hitmin_and_at_the_hitdiff_threshold(eng):
    """the `mini` database's taxonomy; lists whose best entry has exactly hitmin hits and one less, and second entries exactly at,
    just above and just below (h0 - hitmin) * hitdiff"""
    host = importlib.import_module("metacache-mpi_amd.host")
    db = host.RefDb(os.path.join(HERE, "golden", "mini", "P2", "mini"), 2)
    lin, rank = db.lineages()
    ids = [db.taxon_id(t) for t in range(db.info.n_taxa)]
    M = ref.Tax.of_lineages(ids, lin, rank)
    mtax = eng.Taxonomy(lin, rank)
    hits_min, frac, highest = 4, np.float32(0.8), R["family"]
    cases = [[(101, 4)], [(101, 3)], [(101, 5), (102, 5)], [(101, 14), (102, 8)], [(101, 14), (102, 9)], [(101, 14), (201, 9)],
             [(101, 14), (301, 9)], [(101, 9), (102, 4), (301, 4)], [(101, 9), (102, 5), (301, 5)], [(301, 29), (102, 20), (201, 3)],
             [], [(100, 6), (101, 6)], [(30, 9)], [(40, 9), (201, 8)]]
    text = b"".join(line(q + 1, items) for q, items in enumerate(cases))
    m = eng.Merge(mtax, host.taxid_table(db), len(cases), 4)
    assert _feed(m, text)
    n, pairs, _ = m.lists()
    best, counts = m.finish(hits_min, float(frac), highest)
    want = []
    for q in range(len(cases)):
        c = np.zeros((int(n[q]), 4), np.uint32)
        c[:, :2] = pairs[q, :n[q]]
        want.append(db.classify(c, hits_min, float(frac), highest) if len(c) else ref.NONE)
        assert want[-1] == ref.classify([list(map(int, p)) for p in pairs[q, :n[q]]], M, hits_min, frac, highest), q
    assert [int(b) for b in best] == want
    name = lambda b: None if b == ref.NONE else ids[b]
    assert [name(b) for b in want] == [101, None, 100, 101, 100, 40, None, 101, None, 301, None, 100, None, 40]
    assert int(counts.sum()) == len(cases) and int(counts[db.info.n_taxa]) == want.count(ref.NONE)
    assert all(int(counts[t]) == want.count(t) for t in set(want) - {ref.NONE})
    best2, counts2 = m.finish(hits_min, float(frac), highest)                  # the handle stays usable
    assert np.array_equal(best, best2) and np.array_equal(counts, counts2)
    m.close()
    db.close()
