"""The Python restatement of the reference's `annotate taxid` (tests/annotate_ref.py) against the files the reference itself wrote
(tests/golden/annotate, made by tests/golden/make_golden_annotate.py): byte for byte.  No GPU, no native code."""
import gzip
import os

import pytest

import annotate_ref as ar

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "annotate")
TAX = os.path.join(os.path.dirname(GOLDEN), "accmap", "tax")
MAPPINGS = [os.path.join(TAX, n + ".accession2taxid") for n in ("nucl_gb", "nucl_wgs", "extra")]
# (input, recorded output, id type, field separator, value separator)
RUNS = [("in.fa", "in.accver.fa", ar.ACCVER, b" ", b"|"), ("in.fa", "in.acc.fa", ar.ACC, b" ", b"|"), ("in.fa", "in.gi.fa", ar.GI, b" ", b"|"),
        ("in.fa", "in.sep.fa", ar.ACCVER, b"_", b":"), ("gap.fa", "gap.accver.fa", ar.ACCVER, b" ", b"|"),
        ("reads.fq", "reads.accver.fq", ar.ACCVER, b" ", b"|")]


def golden(name):
    with gzip.open(os.path.join(GOLDEN, name + ".gz"), "rb") as f:
        return f.read()


def mapping(id_type):
    m = {}
    for path in MAPPINGS:
        with open(path, "rb") as f:
            ar.read_mappings(f.read(), id_type, m)
    return m


@pytest.mark.parametrize("infile,outfile,id_type,fs,vs", RUNS, ids=[r[1] for r in RUNS])
def test_restatement_writes_what_the_reference_wrote(infile, outfile, id_type, fs, vs):
    assert ar.annotate(golden(infile), mapping(id_type), id_type, fs, vs) == golden(outfile)


def test_the_fixture_holds_the_cases_it_is_there_for():
    text, out = golden("in.fa"), golden("in.accver.fa")
    assert b">NC_000002.1\n" in text and b">NC_000002.1 taxid|101 \n" in out                       # no field separator: appended
    assert b"again taxid|55\n" in text and b">NC_000003.1 taxid|0 again \n" in out                  # old taxid last: cut to the end
    assert b">seq7.1 taxid|0 plasmid\n" in out and b">seq7.1 plasmid\n" in golden("in.acc.fa")      # the id that begins with '>'
    assert ar.header_id(b">seq7.1 plasmid", ar.ACCVER) == b">seq7.1" and ar.header_id(b">seq7.1 plasmid", ar.ACC) == b""
    assert b"crlf\r\n" in text and b">NC_000006.1 taxid|202 crlf\r\n" in out
    assert b">gi|5550008|synthetic taxid|301 \n" in golden("in.gi.fa")
    assert b">NC_taxid:777_000001.1 synthetic\n" in golden("in.sep.fa")                             # one byte behind the FIRST '_'
    assert b"\n\n" in golden("gap.fa") and golden("gap.accver.fa").count(b">") == 2 and not golden("gap.accver.fa").endswith(b"\n")
    fq = golden("reads.accver.fq")
    assert b"\n@II.I" in golden("reads.fq") and b"IIII taxid|0 \n" in fq and fq.endswith(b"\n@" + b"F" * 39)
    m = mapping(ar.ACCVER)
    assert m[b"NC_000001.1"] == 777 and m[b"NC_000006.1"] == 202 and m[b"NC_000009.1"] == 0 and b"NC_000010.1" not in m
