"""The Python restatement of the reference's merge mode (tests/merge_ref.py) against what the reference itself printed for two
hand-made files over the `mini` taxonomy (`merge a.txt b.txt -hitmin 4 -maxcand 4 -tophits -lowest species -queryids`: the
merged top_hits and classifications below are its output), and the lines it does not return from."""
import gzip
import os

import pytest

import merge_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
T = ref.Tax.of_dump(os.path.join(HERE, "golden", "mini", "nodes.dmp"))
HEAD = (b"# Reporting per-read mappings (non-mapping lines start with '# ').\n"
        b"# Only the lowest matching rank will be reported.\n"
        b"# Classification will be constrained to ranks from 'species' to 'domain'.\n"
        b"# Classification hit threshold is 4 per query\n"
        b"# TABLE_LAYOUT: query_id\t|\tquery_header\t|\ttop_hits\t|\trank:taxname\n")


def _line(q, hits, cls=b"species:x"):
    return b"%d\t|\tq%04d\t|\t%s\t|\t%s\n" % (q, q, hits, cls)


A = b"".join([_line(1, b"301:25"), _line(2, b"201:29,202:6"), _line(3, b""), _line(4, b"101:7,102:7")])
B = b"".join([_line(2, b"202:29,301:6,201:3"), _line(1, b"301:20,101:25"), _line(3, b"102:9"), _line(4, b"102:7,999:9")])


def _merged(files, max_cand=4):
    m = ref.Merged(T, 4, max_cand)
    for f in files:
        m.read_results(f)
    return m


def _show(m):
    return [b",".join(b"%d:%d" % (T.ids[t], h) for t, h in l) for l in m.lists]


def test_the_example_the_reference_was_run_on():
    m = _merged([A, B])
    assert _show(m) == [b"301:25,101:25", b"201:29,202:29,301:6", b"102:9", b"101:7,102:7"]
    assert m.unknown == 1 and m.headers == [b"q0001", b"q0002", b"q0003", b"q0004"]
    best = [ref.classify(l, T, 4, 1.0, ref.RANK["domain"]) for l in m.lists]
    assert [T.ids[b] for b in best] == [30, 200, 102, 100]          # order:Ord, genus:GenB, species:GenA two, genus:GenA
    at_or_below = lambda r: sum(1 for b in best if T.rank[b] <= ref.RANK[r])
    assert [at_or_below(r) for r in ("species", "genus", "order")] == [1, 3, 4]


def test_the_order_of_the_files_and_the_comment_lines():
    assert _show(_merged([B, A])) == [b"101:25,301:25", b"202:29,201:29,301:6", b"102:9", b"102:7,101:7"]
    with_comments = b"# in front\n" + A.replace(b"\n3\t", b"\n# between\n3\t") + b"# behind\n#\n"
    assert _show(_merged([with_comments, B])) == _show(_merged([A, B]))
    assert _show(_merged([A, B], 2)) == [b"301:25,101:25", b"201:29,202:29", b"102:9", b"101:7,102:7"]


def test_the_strict_form_of_the_example():
    for text in (A, B, HEAD + A, A[:-1]):
        assert ref.is_strict(text, 4)
    assert not ref.is_strict(A, 3) and not ref.is_strict(A + A, 4) and not ref.is_strict(A + b"\n", 4)
    assert not ref.is_strict(A.replace(b"q0002", b"q0002 taxid|5"), 4)


@pytest.mark.parametrize("bad", [_line(2, b"201:29", b"x").replace(b"q0002", b"q0002 taxid|5"),      # a '|' in the header column
                                 _line(2, b"NC_000913.3:5"),                                             # a sequence name for an item
                                 _line(2, b"201:99999999999999999999"),                                  # hits that overflow
                                 _line(0, b"201:5"), _line(5, b"201:5"), b"\n"])                         # id 0, an id beyond the queries, an empty line at the end
def test_the_lines_the_reference_does_not_return_from(bad):
    text = _line(1, b"301:25") + bad
    assert not ref.is_strict(text, 4)
    with pytest.raises(ref.Stop) as e:
        _merged([text])
    assert e.value.line_no == 2


GOLDEN = os.path.join(HERE, "golden", "merge")


def golden_results():
    """[(mapping part of res_<k>.txt, its top_hits column, its line count)] of tests/golden/merge (make_golden_merge.py)"""
    out = []
    for k in range(3):
        text = gzip.open(os.path.join(GOLDEN, "res_%d.txt.gz" % k), "rb").read()
        head = text[:text.index(b"# TABLE_LAYOUT:")]
        layout = text[len(head):text.index(b"\n", len(head))]
        assert layout.split(b"\t|\t")[0].endswith(b"query_id")
        begin = text.index(b"\n", text.index(b"\n", len(head)) + 1) + 1          # (behind the layout line and the line that names the reads)
        body = text[begin:]
        out.append((body, [c.strip() for c in layout.split(b"\t|\t")].index(b"top_hits"), sum(1 for l in body.split(b"\n") if l and l[:1] != b"#")))
    return out


@pytest.mark.parametrize("name,max_cand,highest", [("tophits", 4, "domain"), ("lineage", 4, "domain"), ("abundance", 4, "domain"), ("genus", 2, "genus")])
def test_the_restatement_against_the_references_merged_files(name, max_cand, highest):
    names = {int(l.split("|")[0]): l.split("|")[1].strip() for l in open(os.path.join(HERE, "golden", "mini", "names.dmp"))}
    files = golden_results()
    assert all(ref.is_strict(body, n, col) for body, col, n in files)      # (what the reference writes is strict)
    m = ref.Merged(T, files[0][2], max_cand)
    for body, col, n in files:
        assert (col, n) == (2, 293)
        m.read_results(body, col)
    merged = gzip.open(os.path.join(GOLDEN, "merged_%s.out.gz" % name), "rt").read()
    got = {}
    for l in merged.split("\n"):
        if l and not l.startswith("#"):
            cols = l.split("\t|\t")
            got[cols[1] if name == "tophits" else cols[0]] = cols
    n_unclassified = 0
    for q in range(293):
        best = ref.classify(m.lists[q], T, 4, 1.0, ref.RANK[highest])
        n_unclassified += best == ref.NONE
        header = m.headers[q].decode()
        if name == "abundance" and best == ref.NONE:
            assert header not in got                                        # (-mapped-only)
            continue
        cols = got[header]
        if name == "tophits":
            assert cols[0] == str(q + 1) and cols[2] == ",".join("%d:%d" % (T.ids[t], h) for t, h in m.lists[q])
        if best == ref.NONE:
            assert cols[-1].startswith("--")
        elif name == "lineage":
            assert cols[-1].split(",")[0] == "%s:%s(%d)" % (ref.RANKS[T.rank[best]], names[T.ids[best]], T.ids[best])
        else:
            assert cols[-1] == "%s:%s" % (ref.RANKS[T.rank[best]], names[T.ids[best]])
    assert "# unclassified: " in merged and "(%d)" % n_unclassified in merged.split("# unclassified: ")[1].split("\n")[0]
