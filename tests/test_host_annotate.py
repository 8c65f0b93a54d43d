"""libmcq_host's part of annotate (include/mcq_host.h: mcq_annotate_id, mcq_annotate_rewrite, mcq_accmap_host_rule) against the Python
restatement tests/annotate_ref.py, and through it against the files the reference wrote (tests/golden/annotate).  No GPU."""
import importlib

import numpy as np
import pytest

import annotate_ref as ar
from test_annotate_ref import MAPPINGS, RUNS, golden


@pytest.fixture(scope="module")
def host():
    pkg = importlib.import_module("metacache-mpi_amd")
    pkg.build_host()
    return importlib.import_module("metacache-mpi_amd.host")


def header_lines():
    """every header line of the three fixture inputs (the CR of the CRLF header stays in its line), and a few more by hand"""
    lines = []
    for name in ("in.fa", "gap.fa", "reads.fq"):
        lines += [l for l in golden(name).split(b"\n") if l[:1] in (b">", b"@")]
    lines += [b">", b">x", b">.", b">a.b", b">" + b"x" * 30 + b".1 late dot", b">NC_ 1", b">gi|", b">gi|12", b">gi|12 x|y", b">taxid", b">taxid|",
              b">a taxid|7", b">a taxid|7|b c", b">a taxid=7 b", b">a  taxid|7  b", b">xtaxi taxid||5||rest", b">AE017.2-x_y,z NC_1.5|q",
              b">GCF_000001.1_a NC_000001.1", b">lcl|CP000001.1_cds_1 [x]", b">NC_0000000000000000000000000.1 far dot", b"@NC_000006.1/1"]
    assert len(lines) > 40
    return lines


SEPS = [(b" ", b"|"), (b"_", b":"), (b"||", b"::"), (b"  ", b"|"), (b" ", b"=|"), (b"ta", b"id")]


def test_the_id_of_a_header_line(host):
    for line in header_lines():
        for t in (ar.ACC, ar.ACCVER, ar.GI):
            assert host.annotate_id(line, t) == ar.header_id(line, t), (line, t)
    assert host.annotate_id(b">seq7.1 plasmid", host.ID_ACCVER) == b">seq7.1"
    assert (host.ID_ACC, host.ID_ACCVER, host.ID_GI) == (ar.ACC, ar.ACCVER, ar.GI)


@pytest.mark.parametrize("fs,vs", SEPS)
def test_the_rewrite_of_a_header_line(host, fs, vs):
    for line in header_lines():
        for has_id, taxid in ((True, 0), (True, 202), (True, 2 ** 64 - 1), (False, 5)):
            assert host.annotate_rewrite(line, has_id, taxid, fs, vs) == ar.rewrite(line, has_id, taxid, fs, vs), (line, has_id, taxid)


def test_rewrite_by_hand(host):
    assert host.annotate_rewrite(b">a b", True, 7) == b">a taxid|7 b"
    assert host.annotate_rewrite(b">ab", True, 7) == b">ab taxid|7 "
    assert host.annotate_rewrite(b">a taxid|1 b", True, 7) == b">a taxid|7 b"
    assert host.annotate_rewrite(b">a taxid|1", True, 7) == b">a taxid|7 "
    assert host.annotate_rewrite(b">a taxid|1 b", False, 7) == b">a b"
    assert host.annotate_rewrite(b">a||b", True, 7, b"||", b"::") == b">a|taxid::7|||b"          # ipos + 1 inside the separator
    with pytest.raises(RuntimeError):
        host.annotate_rewrite(b">a", True, 1, b"", b"|")


TEXTS = {
    "strict": b"h\nA\tA.1\t5\t50\nB\tB.1\t6\t60\nA\tA.1\t7\t70\nC\tC.2\t0\t80\n",
    "blanks_and_records_across_lines": b"skipped line\nA A.1\n5 50\n\n  B\tB.1 6\n60 C C.2 8 80",
    "a_taxid_that_is_no_number_ends_the_file": b"h\nA\tA.1\t5\t50\nB\tB.1\tx\t60\nC\tC.2\t8\t80\n",
    "signed_and_trailing_letters": b"h\nA\tA.1\t+5x\t50\nB\tB.1\t-1\t60\n",
    "ends_inside_a_record": b"h\nA\tA.1\t5\t50\nB\tB.1\t6",
    "beyond_64_bits": b"h\nA\tA.1\t5\t50\nB\tB.1\t18446744073709551616\t60\nC\tC.2\t8\t80\n",
    "crlf": b"h\r\nA\tA.1\t5\t50\r\nC\tC.2\t8\t80\r\n",
    "only_a_first_line": b"accession\taccession.version\ttaxid\tgi",
    "empty": b"",
}
NAMES = [b"A", b"A.1", b"50", b"B.1", b"C", b"80", b"C.2", b"60", b"zz"]


@pytest.mark.parametrize("rule", [ar.ACC, ar.ACCVER, ar.GI])
@pytest.mark.parametrize("case", sorted(TEXTS))
def test_rule_parser_against_the_restatement(host, case, rule):
    for skip in (True, False):
        for ranked in ([], [1, 2]):
            unranked, parent = np.ones(len(NAMES), np.uint8), np.zeros(len(NAMES), np.int64)
            unranked[ranked] = 0
            want_u, want_p = [bool(u) for u in unranked], [0] * len(NAMES)
            n_want = ar.accmap_rule(TEXTS[case], NAMES, want_u, want_p, rule, skip)
            assert host.accmap_host(TEXTS[case], NAMES, unranked, parent, skip, rule=rule) == n_want, (case, skip)
            assert [bool(u) for u in unranked] == want_u and [int(p) for p in parent] == want_p, (case, skip)
    if case == "strict" and rule == ar.ACCVER:                   # (all unranked, first line passed over)
        unranked, parent = np.ones(len(NAMES), np.uint8), np.zeros(len(NAMES), np.int64)
        assert host.accmap_host(TEXTS[case], NAMES, unranked, parent, rule=rule) == 4
        assert list(parent) == [0, 5, 0, 6, 0, 0, 0, 0, 0] and list(unranked) == [1, 0, 1, 0, 1, 1, 0, 1, 1]    # ONE column, the first line wins, a 0 counts


def test_rule_zero_is_the_parser_it_was(host):
    import taxmap_ref as tr
    text = b"h\nNC_1\tNC_1.7\t5\t1\nQ\tQ.1\t9\t777\n"
    names = [b"NC_10.1", b"777", b"NC_1"]
    a_u, a_p = np.ones(3, np.uint8), np.zeros(3, np.int64)
    b_u, b_p = np.ones(3, np.uint8), np.zeros(3, np.int64)
    assert host.accmap_host(text, names, a_u, a_p) == host.accmap_host(text, names, b_u, b_p, rule=0) == 2
    want_u, want_p = [True] * 3, [0] * 3
    tr.accmap(text, tr.Names(names), want_u, want_p)
    assert list(a_p) == list(b_p) == want_p == [5, 9, 0] and list(a_u) == list(b_u)
    with pytest.raises(RuntimeError):
        host.accmap_host(text, names, a_u, a_p, rule=4)


@pytest.mark.parametrize("infile,outfile,id_type,fs,vs", RUNS, ids=[r[1] for r in RUNS])
def test_the_library_writes_what_the_reference_wrote(host, infile, outfile, id_type, fs, vs):
    """the three passes of mcq_annotate_cli with the library's functions alone: ids, join on the host, rewrite"""
    lines = golden(infile).split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    if b"" in lines:
        lines = lines[:lines.index(b"")]
    headers = [l for l in lines if l[:1] in (b">", b"@")]
    ids = sorted({host.annotate_id(l, id_type) for l in headers} - {b""})
    unranked, parent = np.ones(len(ids), np.uint8), np.zeros(len(ids), np.int64)
    for path in MAPPINGS:
        with open(path, "rb") as f:
            host.accmap_host(f.read(), ids, unranked, parent, rule=id_type)
    taxid = {i: int(p) for i, p, u in zip(ids, parent, unranked) if not u}
    out = []
    for l in lines:
        if l[:1] in (b">", b"@"):
            i = host.annotate_id(l, id_type)
            l = host.annotate_rewrite(l, bool(i), taxid.get(i, 0), fs, vs)
        out.append(l)
    assert b"\n".join(out) == golden(outfile)
