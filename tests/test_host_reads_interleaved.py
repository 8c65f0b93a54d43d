"""Interleaved pairs in the host parser (mcq_reads_parse with MCQ_READS_INTERLEAVED, include/mcq_host.h) and the input lists of
the query programs.  Records 2q, 2q+1 of one text are the mates of query q, as the reference's sequence_pair_reader::next
pairs them under -pairseq; whatever the chunk size, the queries must be those the two-text parse of the de-interleaved
files gives, a chunk must never be cut between two mates, and a last record without a mate is a query with an empty
second mate.  The option parser is driven through -list-inputs, which leaves before the database is opened."""
import importlib
import subprocess

import pytest

from interleaved_texts import deinterleave, interleaved_records, render
from read_edge_texts import interleaved_corpus, interleaved_pairs

CHUNKS = list(range(1, 301))
COARSE = [1, 2, 3, 37, 97, 150, 300]          # the even record count differs from the odd one only at the end of the file


@pytest.fixture(scope="module")
def host():
    pkg = importlib.import_module("metacache-mpi_amd")
    pkg.build_host()
    return importlib.import_module("metacache-mpi_amd.host")


def _queries(texts, info, bases, seq_off, hdr):
    n, out = int(info[0]), []
    for q in range(n):
        s = [bytes(bases[int(seq_off[2 * q + m]):int(seq_off[2 * q + m + 1])]) for m in range(2)]
        out.append((texts[0][int(hdr[2 * q]):int(hdr[2 * q + 1])], s[0], s[1]))
    return out


def _expected(host, recs, fmt):
    """the two-text parse of the de-interleaved files, whole; an unpaired last record added as the reference pairs it"""
    t1, t2 = (render(r, fmt, final_newline=True) for r in deinterleave(recs))
    big = 1 << 40
    info, bases, seq_off, hdr = host.parse_chunk([t1, t2], host.READS_EOF1 | host.READS_EOF2, big, 1 << 62)
    exp = _queries([t1, t2], info, bases, seq_off, hdr)
    assert len(exp) == len(recs) // 2
    if len(recs) & 1:
        exp.append((recs[-1][0].split(b" ")[0], recs[-1][1], b""))
    return exp


def _run(host, path, chunk, max_q=1 << 40, max_b=1 << 62):
    got, batches = [], []
    for texts, info, bases, seq_off, hdr, _ in host.read_batches([path], chunk, max_q, max_b, interleaved=True):
        assert len(texts) == 1 and info[host.READS_STATUS] == 0 and info[host.READS_CUT2] == 0 and info[host.READS_COMPLETE2] == 0
        n = int(info[host.READS_N])
        assert 1 <= n <= max_q and int(seq_off[2 * n]) == int(info[host.READS_BASES])
        got += _queries(texts, info, bases, seq_off, hdr)
        batches.append((n, int(info[host.READS_BASES]), texts[0], int(info[host.READS_CUT1])))
    return got, batches


@pytest.mark.parametrize("odd", [False, True])
@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_every_chunk_size_gives_the_pairs_of_the_two_file_parse(host, fmt, odd, tmp_path):
    """the 197 pairs of `mini` with an N read, a lowercase read and its 2 kb reads, no final newline, and a last record
    that has no mate: every chunk size from 1 to 300 bytes; without that record: a coarse set of them"""
    recs = interleaved_records(odd=odd)
    exp = _expected(host, recs, fmt)
    path = tmp_path / "il.txt"
    path.write_bytes(render(recs, fmt, final_newline=False))
    for chunk in (CHUNKS if odd else COARSE) + [4096, 1 << 16]:
        got, _ = _run(host, path, chunk)
        assert got == exp, (fmt, odd, chunk)


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_unpaired_last_record_is_a_query_with_an_empty_second_mate(host, fmt):
    """by hand: three records.  Not at the end of the file the third waits for its mate; at the end it is a query of its own"""
    recs = [(b"a x", b"ACGT"), (b"a/2", b"GG"), (b"b y", b"TTT")]
    t = render(recs, fmt, final_newline=True)
    info, bases, seq_off, hdr = host.parse_chunk([t], host.READS_INTERLEAVED, 100, 1 << 30)
    assert int(info[host.READS_N]) == 1 and int(info[host.READS_COMPLETE1]) == 1
    assert int(info[host.READS_CUT1]) == t.index(b"b y") - 1
    assert _queries([t], info, bases, seq_off, hdr) == [(b"a", b"ACGT", b"GG")]
    info, bases, seq_off, hdr = host.parse_chunk([t], host.READS_INTERLEAVED | host.READS_EOF1, 100, 1 << 30)
    assert int(info[host.READS_N]) == 2 and int(info[host.READS_COMPLETE1]) == 2 and int(info[host.READS_CUT1]) == len(t)
    assert _queries([t], info, bases, seq_off, hdr) == [(b"a", b"ACGT", b"GG"), (b"b", b"TTT", b"")]
    assert seq_off[:5].tolist() == [0, 4, 6, 9, 9]


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_a_chunk_that_ends_between_two_mates_takes_neither(host, fmt):
    recs = [(b"a", b"ACGT"), (b"a/2", b"GG"), (b"b", b"TTT"), (b"b/2", b"CCCC")]
    t = render(recs, fmt, final_newline=True)
    at_b, at_b2 = t.index(b"b\n") - 1, t.index(b"b/2") - 1
    for end in range(at_b + 1, at_b2 + 2):          # up to the first byte of b/2: record b is complete at the most
        info, *_ = host.parse_chunk([t[:end]], host.READS_INTERLEAVED, 100, 1 << 30)
        assert int(info[host.READS_N]) == 1 and int(info[host.READS_CUT1]) == at_b, end
    info, *_ = host.parse_chunk([t], host.READS_INTERLEAVED, 100, 1 << 30)
    assert int(info[host.READS_N]) == 1                         # b/2 is complete only with the byte that follows it
    info, *_ = host.parse_chunk([t + (b"@" if fmt == "fastq" else b">")], host.READS_INTERLEAVED, 100, 1 << 30)
    assert int(info[host.READS_N]) == 2 and int(info[host.READS_CUT1]) == len(t)


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
@pytest.mark.parametrize("chunk", [97, 4096])
@pytest.mark.parametrize("max_q,max_b", [(1, 1 << 62), (2, 1 << 62), (3, 1 << 62), (1 << 40, 20), (4, 400)])
def test_limits_count_pairs_and_cuts_fall_in_front_of_a_first_mate(host, fmt, chunk, max_q, max_b, tmp_path):
    """max_queries counts pairs, max_bases the bases of both mates (20 is less than any pair of `mini`: every pair goes
    alone); nothing is lost or doubled, and every cut lies at the header of a first mate or at the end of the text"""
    recs = interleaved_records(odd=True)[:2 * 40 + 1]
    exp = _expected(host, recs, fmt)
    path = tmp_path / "il.txt"
    path.write_bytes(render(recs, fmt, final_newline=False))
    got, batches = _run(host, path, chunk, max_q, max_b)
    assert got == exp
    whole, starts = render(recs, fmt, final_newline=False), set()
    for h, _ in recs[0::2]:
        starts.add(whole.index((b"@" if fmt == "fastq" else b">") + h + b"\n"))
    at = 0                                           # where the batch's text begins in the file
    for n, nb, text, cut in batches:
        assert n <= max_q and (nb <= max_b or n == 1), (n, nb)
        at += cut
        assert at in starts or at == len(whole), (at, whole[at:at + 30])
    if max_b == 20:
        assert all(n == 1 for n, *_ in batches)


@pytest.mark.parametrize("name", sorted(interleaved_corpus()))
def test_interleaved_texts_of_the_device_tests_against_read_records(host, name, tmp_path):
    """the texts tests/test_gpu_reads_prepare_edges.py runs the device step on (CRLF ones included): the queries are the
    records of read_records paired two by two, whatever the chunk size"""
    text, _strict = interleaved_corpus()[name]
    path = tmp_path / "il.txt"
    path.write_bytes(text)
    exp = interleaved_pairs(text)
    for chunk in COARSE + [4096, 1 << 20]:
        got, _ = _run(host, path, chunk)
        assert got == exp, (name, chunk)


def _list(pkg, args, cwd):
    r = subprocess.run([pkg.cli_path(), "no_such_db", "4"] + args + ["-list-inputs"], cwd=cwd, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=60)
    return r.returncode, r.stdout.split("\n")[:-1], r.stderr


def test_input_lists_of_the_command_line(tmp_path):
    pkg = importlib.import_module("metacache-mpi_amd")
    pkg.build_host()
    # today's two forms, unchanged: one pair in the given order, one single-end file
    assert _list(pkg, ["z.fq", "a.fq"], tmp_path)[:2] == (0, ["pairing: files", "z.fq + a.fq"])
    assert _list(pkg, ["z.fq", "-"], tmp_path)[:2] == (0, ["pairing: none", "z.fq"])
    assert _list(pkg, ["z.fq", "a.fq", "-pairfiles"], tmp_path)[:2] == (0, ["pairing: files", "z.fq + a.fq"])
    # -pairfiles: sorted, consecutive names paired; an odd count refused
    names = ["s3_2.fq", "s1_1.fq", "s2_2.fq", "s1_2.fq", "s3_1.fq", "s2_1.fq"]
    assert _list(pkg, names + ["-pairfiles"], tmp_path)[:2] == (0, ["pairing: files", "s1_1.fq + s1_2.fq", "s2_1.fq + s2_2.fq", "s3_1.fq + s3_2.fq"])
    for alias in ("-pair-files", "-paired_files"):
        assert _list(pkg, names + [alias], tmp_path)[1][0] == "pairing: files"
    rc, out, err = _list(pkg, names[:5] + ["-pairfiles"], tmp_path)
    assert rc != 0 and out == [] and "even number" in err
    # without a pairing option: single-end files in the given order; -pairseq: every file interleaved
    assert _list(pkg, names[:3], tmp_path)[:2] == (0, ["pairing: none"] + names[:3])
    assert _list(pkg, names[:3] + ["-pairseq"], tmp_path)[:2] == (0, ["pairing: sequences"] + names[:3])
    assert _list(pkg, names[:1] + ["-paired"], tmp_path)[:2] == (0, ["pairing: sequences"] + names[:1])
    # ... also exactly two names, or one and "-"; -pairfiles, if given too, comes first (src/query_options.cpp:83-97)
    assert _list(pkg, ["z.fq", "a.fq", "-pairseq"], tmp_path)[:2] == (0, ["pairing: sequences", "z.fq", "a.fq"])
    assert _list(pkg, ["z.fq", "-", "-pairseq"], tmp_path)[:2] == (0, ["pairing: sequences", "z.fq"])
    assert _list(pkg, ["z.fq", "a.fq", "-pairseq", "-pairfiles"], tmp_path)[:2] == (0, ["pairing: files", "z.fq + a.fq"])
    assert _list(pkg, names[:4] + ["-pairfiles", "-pairseq"], tmp_path)[:2] == (0, ["pairing: files", "s1_1.fq + s1_2.fq", "s2_2.fq + s3_2.fq"])
    # a directory stands for its files (subdirectories included); the options end the inputs
    d = tmp_path / "lanes"
    (d / "sub").mkdir(parents=True)
    for n in ("b_2.fq", "a_1.fq", "sub/c_1.fq", "a_2.fq", "sub/c_2.fq", "b_1.fq"):
        (d / n).write_bytes(b"")
    files = ["lanes/" + n for n in ("a_1.fq", "a_2.fq", "b_1.fq", "b_2.fq", "sub/c_1.fq", "sub/c_2.fq")]
    assert _list(pkg, ["lanes", "-pairfiles", "-out", "o.txt"], tmp_path)[:2] == (0, ["pairing: files"] + [a + " + " + b for a, b in zip(files[0::2], files[1::2])])
    assert _list(pkg, ["lanes/"], tmp_path)[:2] == (0, ["pairing: none"] + files)
    # -splitout: one output per unit, named by the prefix and the file names without their directories
    assert _list(pkg, ["lanes", "-pairfiles", "-splitout", "res"], tmp_path)[1][1:] == \
        ["lanes/a_1.fq + lanes/a_2.fq\tres_a_1.fq_a_2.fq.txt", "lanes/b_1.fq + lanes/b_2.fq\tres_b_1.fq_b_2.fq.txt", "lanes/sub/c_1.fq + lanes/sub/c_2.fq\tres_c_1.fq_c_2.fq.txt"]
    assert _list(pkg, ["x.fq", "y.fq", "w.fq", "-split-out", "-out", "res"], tmp_path)[1][1:] == ["x.fq\tres_x.fq.txt", "y.fq\tres_y.fq.txt", "w.fq\tres_w.fq.txt"]
    # no input at all: the usage, nothing else
    r = subprocess.run([pkg.cli_path(), "no_such_db", "4", "-pairfiles"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert r.returncode == 2 and r.stdout == "" and "usage" in r.stderr
