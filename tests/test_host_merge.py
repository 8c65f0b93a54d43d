"""The host side of merging result files (libmcq_host: mcq_results_properties, mcq_merge_host, mcq_refdb_from_taxdump,
mcq_refdb_taxid_table) against the Python restatement of the reference (tests/merge_ref.py) and the `mini` taxonomy."""
import importlib
import os
import random

import numpy as np
import pytest

import merge_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
MINI = os.path.join(HERE, "golden", "mini")
T = ref.Tax.of_dump(os.path.join(MINI, "nodes.dmp"))
HEAD = (b"# Reporting per-read mappings (non-mapping lines start with '# ').\n"
        b"# Only the lowest matching rank will be reported.\n"
        b"# Classification will be constrained to ranks from 'species' to 'domain'.\n"
        b"# Classification hit threshold is 4 per query\n")
LAYOUT = b"# TABLE_LAYOUT: query_id\t|\tquery_header\t|\ttop_hits\t|\trank:taxname\n"


@pytest.fixture(scope="module")
def host():
    return importlib.import_module("metacache-mpi_amd.host")


def _line(q, hits, header=None):
    return b"%d\t|\t%s\t|\t%s\t|\tspecies:x\n" % (q, b"q%04d" % q if header is None else header, hits)


BODY = b"".join([_line(1, b"301:25"), _line(2, b"201:29,202:6"), _line(3, b""), _line(4, b"101:7,102:7")])


def _write(tmp_path, text, name="r.txt"):
    p = tmp_path / name
    p.write_bytes(text)
    return str(p)


def test_properties_of_a_results_file(host, tmp_path):
    assert host.results_properties(_write(tmp_path, HEAD + LAYOUT + BODY)) == (2, len(HEAD + LAYOUT), 4)
    more = HEAD + LAYOUT + b"# one more comment\n#\n" + BODY.replace(b"\n3\t", b"\n# between\n3\t") + b"# behind\n"
    assert host.results_properties(_write(tmp_path, more)) == (2, len(HEAD + LAYOUT) + 21, 4)
    wide = LAYOUT.replace(b"top_hits", b"query_length\t|\ttop_hits")
    assert host.results_properties(_write(tmp_path, HEAD + wide + BODY[:-1] + b"\n\n"))[::2] == (3, 5)      # (an empty line counts)
    assert host.results_properties(_write(tmp_path, HEAD + LAYOUT)) == (2, len(HEAD + LAYOUT), 0)
    assert host.results_properties(_write(tmp_path, HEAD + LAYOUT[:-1])) == (2, len(HEAD + LAYOUT) - 1, 0)


@pytest.mark.parametrize("text,why", [
    (b"1\t|\tq\t|\t5:5\t|\n", "classification ranks not found"),
    (b"# Reporting\n", "classification ranks not found"),
    (b"", "classification ranks not found"),
    (HEAD.replace(b"'species'", b"'sequence'") + LAYOUT + BODY, "sequence level"),
    (HEAD + BODY, "TABLE_LAYOUT not found"),
    (HEAD, "TABLE_LAYOUT not found"),
    (HEAD + LAYOUT.replace(b"query_id\t|\t", b"") + BODY, "no query_id"),
    (HEAD + LAYOUT.replace(b"top_hits\t|\t", b"") + BODY, "no top_hits"),
])
def test_properties_rejections(host, tmp_path, text, why):
    path = _write(tmp_path, text)
    with pytest.raises(RuntimeError) as e:
        host.results_properties(path)
    assert why in str(e.value) and path in str(e.value)
    with pytest.raises(RuntimeError):
        host.results_properties(path + ".none")


def _want(text, n_queries, column=2):
    m = ref.Merged(T, n_queries, 4)
    m.record = []
    m.read_results(text, column)
    return m.record


def _same(got, want):
    q, off, tid, hits, ho, hl = got
    assert len(q) == len(want) and len(off) == len(q) + 1
    for l, (qid, at, token, items) in enumerate(want):
        assert (int(q[l]), int(ho[l]), int(hl[l])) == (qid, at, len(token))
        assert list(zip(tid[int(off[l]):int(off[l + 1])].tolist(), hits[int(off[l]):int(off[l + 1])].tolist())) == items


LOOSE = [BODY, b"# c\n" + BODY + b"#", BODY[:-1],
         b"".join(l.replace(b"\t|\t", b" | \t", 2) + b"\n" for l in BODY.split(b"\n")[:-1]),      # blanks around the bars in front of top_hits
         b"\n\n" + BODY.replace(b"\n2", b"\n\n  +2"),                 # empty lines and a sign in front of an id
         _line(1, b"-5:7, 101:3;102:4"),                              # a negative taxid, a blank behind a comma, another separator
         _line(2, b"101:5", header=b"  two words") + _line(2, b"102:4294967295"),
         b"1\t|\tq\t|\tlen\t|\t\t|\t101:5\t|\n" * 2]


@pytest.mark.parametrize("k", range(len(LOOSE)))
def test_the_host_parser_reads_what_the_reference_reads(host, k):
    column = 4 if k == len(LOOSE) - 1 else 2
    want = _want(LOOSE[k], 4, column)
    assert want and not (k in (3, 4, 5, 6) and ref.is_strict(LOOSE[k], 4, column))
    _same(host.merge_host(LOOSE[k], 4, column, text_offset=0), want)


def test_offsets_and_random_lines(host):
    rng = random.Random(3)
    text = b"".join(_line(rng.randrange(1, 50), b",".join(b"%d:%d" % (rng.choice(T.ids + [999]), rng.randrange(1, 10 ** rng.randrange(1, 10)))
                                                              for _ in range(rng.randrange(0, 9)))) for _ in range(300))
    got = host.merge_host(text, 49, text_offset=1000)
    want = _want(text, 49)
    _same((got[0], got[1], got[2], got[3], got[4] - 1000, got[5]), want)


STOPS = {
    "a_bar_in_the_header_column": (_line(2, b"201:29", header=b"q0002 taxid|5"), 2),
    "a_bar_in_the_header_token": (_line(2, b"201:29", header=b"q|2"), 2),
    "an_item_that_is_a_name": (_line(2, b"NC_000913.3:5"), 2),
    "hits_that_overflow": (_line(2, b"201:99999999999999999999"), 2),
    "hits_of_two_to_the_32": (_line(2, b"201:4294967296"), 2),
    "an_id_of_zero": (_line(0, b"201:5"), 2),
    "an_id_beyond_the_queries": (_line(5, b"201:5"), 2),
    "a_negative_id": (b"-" + _line(2, b"201:5"), 2),
    "no_id": (b"x" + _line(2, b"201:5"), 2),
    "an_empty_line_at_the_end": (b"\n", 2),
    "a_line_that_ends_in_the_header": (b"2\t|\tq", 2),
    "a_text_that_ends_in_the_items": (b"2\t|\tq\t|\t201:5", 2),
    "a_text_that_ends_behind_a_comma": (b"2\t|\tq\t|\t201:5,", 2),
    "no_top_hits_column": (b"2\t|\tq\n", 2),
    "a_stop_in_the_third_line": (_line(2, b"201:5") + _line(3, b"x:1"), 3),
}


@pytest.mark.parametrize("what", sorted(STOPS))
def test_the_host_parser_stops_where_the_reference_does_not_return(host, what):
    text, line_no = _line(1, b"301:25") + STOPS[what][0], STOPS[what][1]
    with pytest.raises(ref.Stop) as stop:
        _want(text, 4)
    assert stop.value.line_no == line_no
    with pytest.raises(RuntimeError) as e:
        host.merge_host(text, 4, file_name="some/file.txt")
    assert str(e.value).startswith("some/file.txt: line %d: " % line_no)
    with pytest.raises(RuntimeError) as e:
        host.merge_host(text, 4, file_name="f", first_line_no=101)
    assert str(e.value).startswith("f: line %d: " % (line_no + 100))


def test_the_taxonomy_only_database_is_the_mini_taxonomy(host):
    db = host.taxonomy_db(MINI)
    full = host.RefDb(os.path.join(MINI, "P2", "mini"), 2)
    assert db.info.n_targets == 0 and db.info.n_taxa == len(T.ids)
    lin, rank = db.lineages()
    assert np.array_equal(lin, T.lineage) and np.array_equal(rank, T.rank)
    assert [db.taxon_id(t) for t in range(db.info.n_taxa)] == T.ids
    by_id = {full.taxon_id(t): t for t in range(full.info.n_taxa)}
    flin, _ = full.lineages()
    for t, i in enumerate(T.ids):                                # names, ranks, parents and lineages of the database built with the dump
        f = by_id[i]
        assert (db.taxon_name(t), db.taxon_rank(t), db.taxon_parent(t)) == (full.taxon_name(f), full.taxon_rank(f), full.taxon_parent(f))
        assert [ref.NONE if x == ref.NONE else full.taxon_id(int(x)) for x in flin[f]] == [ref.NONE if x == ref.NONE else T.ids[int(x)] for x in lin[t]]
        assert db.ancestor(t, ref.RANK["genus"]) == int(T.lineage[t, ref.RANK["genus"]])
    ids, idx = host.taxid_table(db)
    assert ids.tolist() == sorted(T.ids) and [T.ids[i] for i in idx] == ids.tolist()
    fids, fidx = host.taxid_table(full)
    assert np.all(np.diff(fids) > 0) and [full.taxon_id(int(i)) for i in fidx] == fids.tolist() and len(fids) == full.info.n_taxa
    c = np.array([[T.index[101], 7, 0, 0], [T.index[102], 7, 0, 0]], np.uint32)
    assert db.classify(c, 4, 1.0, ref.RANK["domain"]) == T.index[100] == ref.classify([[int(x[0]), int(x[1])] for x in c], T, 4, 1.0, 19)
    db.close(); full.close()
