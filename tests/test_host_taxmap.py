"""The host side of the mapping of sequences to taxa (include/mcq_host.h: mcq_seq2tax_*, mcq_genome_reader_open_mapped,
mcq_taxmap_files, mcq_accmap_host) against the Python restatement of the reference (tests/taxmap_ref.py), and, on the `accmap`
fixture, against the parents in the files the reference wrote.  No GPU."""
import importlib
import os

import numpy as np
import pytest

import taxmap_inputs as ti
import taxmap_ref as ref


@pytest.fixture(scope="module")
def host():
    pkg = importlib.import_module("metacache-mpi_amd")
    pkg.build_host()
    return importlib.import_module("metacache-mpi_amd.host")


SUMMARY = (b"#   See the README\n# assembly_accession\tbioproject\tbiosample\twgs_master\trefseq_category\ttaxid\tspecies_taxid\n"
           b"GCF_000001.1\tPRJNA1\tSAMN01\t\trepresentative genome\t101\t101\nGCF_000002.1\tPRJNA2\tSAMN02\t\tna\t102\t102\n"
           b"GCF_000001.1\tPRJNA3\tSAMN03\t\tna\t999\t999\n")
FORMS = {
    "ncbi_two_comment_lines": SUMMARY,
    "no_final_newline": SUMMARY[:-1],
    "header_without_comment_lines": b"accession\taccession.version\ttaxid\tgi\nA1\tA1.1\t7\t70\nA2\tA2.1\t8\t80\n",   # (key: the FIRST column)
    "key_column_behind_the_first": b"# x\ty\taccession.version\ttaxid\nq\tr\tK1.1\t5\nq\tr\tK2.1\t6\n",
    "two_columns": b"NC_000004.1\t201\nNC_000004.1\t998\nXY_000001.1\t5\n",
    "two_columns_with_a_comment_line": b"# made by hand\nNC_1.1\t4\nNC_2.1\t5\n",      # "#" -> made: not a number, 0, the file ends
    "taxid_that_is_no_number": b"A.1\t5\nB.1\tfive\nC.1\t6\n",
    "a_short_line_shifts_the_passes": b"# assembly_accession\ta\ttaxid\nG1\tx\t11\nG2\nG3\ty\t13\nG4\tz\t14\n",
    "last_line_without_a_taxid": b"A.1\t5\nB.1",
    "negative_and_signed": b"A.1\t-5\nB.1\t+6\n",
    "eleven_comment_lines": b"".join(b"# c%d\n" % i for i in range(11)) + b"A.1\t5\n",
    "only_comment_lines": b"# a\n# b\n",
    "empty": b"",
    "crlf": b"A.1\t5\r\nB.1\t6\r\n",
}


@pytest.mark.parametrize("form", sorted(FORMS))
def test_mapping_file_reader_against_the_restatement(host, form, tmp_path):
    """every entry (key, taxid) in key order, and find_taxon_id on every key, every proper prefix of a key and a few names that are
    in no file"""
    path = tmp_path / "assembly_summary.txt"
    path.write_bytes(FORMS[form])
    m = host.Seq2Tax()
    assert m.add_file(path) and not m.add_file(tmp_path / "missing.txt")
    want = {}
    ref.read_mapping(FORMS[form], want)
    assert m.items() == sorted(want.items()), form
    probes = set(want) | {k[:i] for k in want for i in range(1, len(k))} | {b"A", b"Z", b"NC_000004.1", b"NC_000004", b"GCF_000001", b"zz"}
    for p in sorted(probes):
        assert m.find(p) == ref.find_taxon_id(want, p), (form, p)
    if form == "ncbi_two_comment_lines":
        assert want == {b"GCF_000001.1": 101, b"GCF_000002.1": 102}
    if form == "two_columns":
        assert want == {b"NC_000004.1": 201, b"XY_000001.1": 5}


def test_the_first_entry_of_a_key_stays_across_files_and_directories_come_in_set_order(host, tmp_path):
    for d, text in (("b", b"K.1\t1\nB.1\t2\n"), ("a", b"K.1\t3\nA.1\t4\n"), ("c", None)):
        os.makedirs(tmp_path / d)
        if text is not None:
            (tmp_path / d / "assembly_summary.txt").write_bytes(text)
    files = [str(tmp_path / "b" / "x.fna"), str(tmp_path / "c" / "y.fna"), str(tmp_path / "a" / "z.fna"), str(tmp_path / "b" / "w.fna"), "plain.fna"]
    m = host.read_seq2tax_for(files)
    assert m.items() == [(b"A.1", 4), (b"B.1", 2), (b"K.1", 3)]                   # a before b: K.1 is a's
    assert ref.unique_directories(files) == sorted({str(tmp_path / d) for d in "abc"} | {"plain.fna"})
    m2 = host.read_seq2tax([tmp_path / "b", tmp_path / "a"])                      # (the order given)
    assert dict(m2.items())[b"K.1"] == 1


MAP = b"""accession\taccession.version\ttaxid\tgi
NC_1\tNC_1.1\t11\t901
NC_5\tNC_5.2\t55\t905
ZZ_9\tZZ_9.1\t99\t777
NC_3\tNC_3.1\t0\t903
NC_3\tNC_3.1\t33\t903
NC_2\tNC_1.1\t22\t902
NC_1\tNC_1.3\t12\t901
"""
NAMES = [b"NC_1.1", b"NC_10.1", b"NC_2.1", b"NC_3.1", b"NC_5.1", b"777", b"NC_7", b"NC_8.1"]
CASES = {
    "plain": MAP,
    "a_short_line_shifts_the_tokens": MAP.replace(b"ZZ_9\tZZ_9.1\t99\t777\n", b"ZZ_9\tZZ_9.1\t99\n"),
    "a_third_token_that_is_no_number_ends_the_file": MAP.replace(b"\t0\t903", b"\tzero\t903"),
    "digits_then_letters_split_a_token": MAP.replace(b"\t55\t905", b"\t55x\t905"),
    "crlf": MAP.replace(b"\n", b"\r\n"),
    "no_final_newline": MAP[:-1],
    "a_header_line_that_looks_like_data": MAP[MAP.index(b"\n") + 1:],
    "blank_lines_and_spaces": MAP.replace(b"\t", b"  ").replace(b"NC_5 ", b"\n\nNC_5 "),
    "a_negative_taxid": MAP.replace(b"\t11\t", b"\t-11\t"),
    "a_taxid_beyond_64_bits_ends_the_file": MAP.replace(b"\t55\t", b"\t18446744073709551616\t"),
    "the_largest_taxid": MAP.replace(b"\t55\t", b"\t18446744073709551615\t"),
    "only_a_header": b"accession\taccession.version\ttaxid\tgi",
    "empty": b"",
}


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("ranked", [(), (0,), (0, 1, 2, 3, 4, 6, 7)])
def test_accmap_host_against_the_restatement(host, case, ranked):
    """the parents, what stays unranked and the number of records read; `ranked`: targets that have a parent beforehand (with all
    but 777 ranked the parser stops at the line that ranks it)"""
    text = CASES[case]
    unranked = np.array([t not in ranked for t in range(len(NAMES))], np.uint8)
    parent = np.array([0 if u else 4242 for u in unranked], np.int64)
    want_u, want_p = [bool(u) for u in unranked], [int(p) for p in parent]
    n_want = ref.accmap(text, ref.Names(NAMES), want_u, want_p)
    n = host.accmap_host(text, NAMES, unranked, parent)
    assert (n, [bool(u) for u in unranked], [int(p) for p in parent]) == (n_want, want_u, want_p), case
    if case == "plain" and not ranked:
        # NC_1.1 by accver; NC_5.1 by acc (NC_5.2 names nobody); 777 by gi; NC_3.1 keeps its FIRST line (taxid 0); NC_2.1: the line
        # whose acc would name it names NC_1.1 by accver; NC_10.1 is not found through NC_1 (NC_1.1 comes first)
        assert want_p == [11, 0, 0, 0, 55, 99, 0, 0] and want_u == [False, True, True, False, False, False, True, True]


def test_accmap_host_in_the_middle_of_a_file_reads_its_first_line(host):
    rest = MAP[MAP.index(b"\n") + 1:]
    for skip in (True, False):
        unranked, parent = np.ones(len(NAMES), np.uint8), np.zeros(len(NAMES), np.int64)
        want_u, want_p = [True] * len(NAMES), [0] * len(NAMES)
        assert host.accmap_host(rest, NAMES, unranked, parent, skip_first_line=skip) == ref.accmap(rest, ref.Names(NAMES), want_u, want_p, skip)
        assert [int(p) for p in parent] == want_p and (want_p[0] == 11) == (not skip)


def test_the_order_of_the_mapping_files(host, tmp_path):
    """-taxpostmap first, the four standard names whether they exist or not, then the others below the directory by name; a name
    that is already in the list is not repeated"""
    tax = tmp_path / "tax"
    os.makedirs(tax / "sub")
    for n in ("zeta.accession2taxid", "nucl_wgs.accession2taxid", "alpha.accession2taxid.gz", "nodes.dmp", "sub/deep.accession2taxid", "nucl_gb.accession2taxid"):
        (tax / n).write_bytes(b"")
    t = str(tax)
    std = [t + "/nucl_%s.accession2taxid" % n for n in ("gb", "wgs", "est", "gss")]
    others = [t + "/alpha.accession2taxid.gz", t + "/sub/deep.accession2taxid", t + "/zeta.accession2taxid"]
    assert host.taxmap_files(t, "my.map") == ["my.map"] + std + others
    assert host.taxmap_files(t + "/", None) == std + others
    assert host.taxmap_files(None, "my.map") == ["my.map"] and host.taxmap_files("", None) == []
    assert host.taxmap_files(t, t + "/zeta.accession2taxid") == [t + "/zeta.accession2taxid"] + std + others[:2]
    assert ti.map_file_order(str(tmp_path), "tax", "my.map") == ["my.map"] + [os.path.relpath(f, str(tmp_path)) for f in std + others]


def _targets_through_the_library(host, work, taxdir="tax", postmap=None, after=None, targets_before=()):
    """what a build does with the library on the host alone: pre-map, genome reader, then mcq_accmap_host over the files that open"""
    cwd = os.getcwd()
    os.chdir(work)
    try:
        files = host.genome_files(["genomes"])
        _, recs, _, _ = host.read_genomes(files, 1 << 20, after=after, seq2tax=host.read_seq2tax_for(files))
        targets = list(targets_before) + [(r["name"].encode("latin-1"), r["parent"]) for r in recs]
        names = [t[0] for t in targets]
        parent = np.array([t[1] for t in targets], np.int64)
        unranked = (parent == 0).astype(np.uint8)
        for f in host.taxmap_files(taxdir, postmap):
            if os.path.isfile(f) and unranked.any():
                host.accmap_host(open(f, "rb").read(), names, unranked, parent)
        return list(zip(names, [int(p) for p in parent]))
    finally:
        os.chdir(cwd)


def test_the_golden_parents(host, tmp_path):
    """pre-mapping plus mcq_accmap_host give every target of the `accmap` fixture the parent the reference's own files hold; so
    does the restatement; and the fixture shows every situation it was made for"""
    work = ti.lay_out(str(tmp_path / "w"))
    gold = ti.golden_targets(host)
    assert gold == [(b"NC_000001.1", 101), (b"NC_000002.1", 101), (b"NC_000003.1", 102), (b"NC_000004.1", 201), (b"NC_000005.1 taxid", 201),
                    (b"NC_000006.1", 202), (b"NC_000007.1", 202), (b"5550008", 301), (b"NC_000009.1", 0), (b"NC_000010.1", 0)]
    assert ti.expected_targets(work) == gold
    assert _targets_through_the_library(host, work) == gold


def test_layouts_without_some_of_the_files(host, tmp_path):
    """no assembly summaries: targets 1 and 2 are found in nucl_wgs, target 0 by the nucl_gb line that names it with 777 (it comes
    first); no *.accession2taxid files: only the pre-mapping and the header;
    neither: the header's taxid|N alone, as before"""
    for tag, kw in (("nosum", dict(summaries=False)), ("nomaps", dict(maps=False)), ("neither", dict(summaries=False, maps=False))):
        work = ti.lay_out(str(tmp_path / tag), **kw)
        want = ti.expected_targets(work)
        assert _targets_through_the_library(host, work) == want, tag
        parents = [p for _, p in want]
        assert parents == {"nosum": [777, 101, 102, 0, 201, 202, 202, 301, 0, 0], "nomaps": [101, 101, 102, 201, 201, 0, 0, 0, 0, 0],
                           "neither": [0, 0, 0, 0, 201, 0, 0, 0, 0, 0]}[tag]
