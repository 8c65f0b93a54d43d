"""tests/align_ref.py, the restatement the GPU tests compare against, held to what the reference itself gave: every recorded
(query, subject) of tests/golden/align/cases.json.gz, and every alignment block of the reference's `-align` run on the mini
fixture (tests/golden/mini/P4/cli_align.out.gz; both made by tests/golden/make_golden_alignment.py)."""
import gzip
import json
import os
import re

import pytest

import align_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TGT_WINLEN = 128            # target window length of the mini fixture (the reference's default)


def load_cases():
    with gzip.open(os.path.join(GOLDEN, "align", "cases.json.gz"), "rt") as f:
        return [(q.encode(), s.encode(), sc, aq.encode(), asub.encode()) for q, s, sc, aq, asub in json.load(f)]


def load_blocks(name="cli_align.out.gz"):
    """{read header: (score, file, index, range begin, range end, aligned query, aligned target)} of a recorded -out file"""
    with gzip.open(os.path.join(GOLDEN, "mini", "P4", name), "rt") as f:
        lines = f.read().split("\n")
    out = {}
    for i, l in enumerate(lines):
        m = re.match(r"#   score  (-?\d+)  aligned to (.*) #(\d+) in range \[(\d+),(\d+)\]$", l)
        if m:
            assert lines[i + 1].startswith("#   query  ") and lines[i + 2].startswith("#   target ")
            out[lines[i - 1].split("\t|\t")[0]] = (int(m.group(1)), m.group(2), int(m.group(3)), int(m.group(4)), int(m.group(5)),
                                                    lines[i + 1][len("#   query  "):].encode(), lines[i + 2][len("#   target "):].encode())
    return out


def load_genomes():
    with gzip.open(os.path.join(GOLDEN, "mini", "genomes.fa.gz"), "rt") as f:
        recs = f.read().split(">")[1:]
    return ["".join(r.split("\n")[1:]).encode() for r in recs]


def load_reads():
    with open(os.path.join(GOLDEN, "mini", "queries.json")) as f:
        q = json.load(f)
    return {n: (a.encode(), b.encode()) for n, a, b in zip(q["names"], q["r1"], q["r2"])}


def test_recorded_cases_cover_the_shapes():
    cases = load_cases()
    ql, sl = {len(c[0]) for c in cases}, {len(c[1]) for c in cases}
    assert {0, 1, 2, 7, 8, 9, 63, 64, 65} <= ql
    assert {0, 1, 63, 64, 65, 127, 128, 129, 511, 512, 513, 4096} <= sl
    assert any(len(c[0]) == 65 and len(c[1]) == 4096 for c in cases)
    assert min(c[2] for c in cases) == -1


def test_restatement_equals_every_recorded_case():
    for q, s, score, aq, asub in load_cases():
        got = align_ref.align_semi_global(q, s)
        assert got == (score, aq, asub), (q[:40], len(q), len(s), got[0], score)
        assert align_ref.align_semi_global(q, s, backtrace=False)[0] == score


def test_minus_one_and_empty():
    assert align_ref.align_semi_global(b"A", b"C") == (-1, b"A", b"C")
    assert align_ref.align_semi_global(b"AC", b"G")[0] == -1
    assert align_ref.align_semi_global(b"", b"ACGT") == (0, b"_", b"_")
    assert align_ref.align_semi_global(b"ACGT", b"") == (0, b"_", b"_")


def test_reverse_complement_changes_acgt_only():
    assert align_ref.reverse_complement(b"ACGTacgtNnRy-") == b"-yRnNacgtACGT"


def test_orientation_reproduces_every_block_of_the_reference_run():
    blocks, genomes, reads = load_blocks(), load_genomes(), load_reads()
    assert len(blocks) == 132
    n_rev = 0
    for name, (score, fname, index, beg, end, aq, at) in blocks.items():
        assert (fname, beg, end) == ("genomes/all.fna", 0, 113)          # the MPI program aligns to window 0 of the top target
        subject = genomes[index - 1][:TGT_WINLEN]
        r1, r2 = reads[name]
        got = align_ref.make_semi_global_alignment(r1, r2, subject)
        assert got[:3] == (score, aq, at), (name, got, score)
        n_rev += got[3]
    assert 0 < n_rev < len(blocks)              # both orientations occur


def test_a_negative_forward_sum_is_a_huge_number():
    """forward sum -1, reverse sum positive: as std::size_t the forward sum is the larger one, and forward is picked"""
    seq1, seq2, subject = b"C", b"", b"G"
    assert align_ref.align_semi_global(seq1, subject)[0] == -1
    assert align_ref.align_semi_global(align_ref.reverse_complement(seq1), subject)[0] == 2
    assert align_ref.make_semi_global_alignment(seq1, seq2, subject) == (-1, b"C", b"G", 0)
    # the same through a pair: both forward scores are -1, the reverse sum is positive
    seq1, seq2, subject = b"AC", b"T", b"G"
    f = align_ref.align_semi_global(seq1, subject)[0] + align_ref.align_semi_global(seq2, subject, False)[0]
    r = align_ref.align_semi_global(b"GT", subject)[0] + align_ref.align_semi_global(b"A", subject, False)[0]
    assert f < 0 < r, (f, r)
    assert align_ref.make_semi_global_alignment(seq1, seq2, subject)[3] == 0
    # a tie goes to reverse
    assert align_ref.make_semi_global_alignment(b"AT", b"", b"AT")[3] == 1
