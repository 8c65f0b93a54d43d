"""Read files for the chunked input stage of mcq_query_cli (tests/test_host_read_stream.py, tests/test_gpu_read_stream.py),
and a Python restatement of the reader they must agree with: read_records of metacache-mpi_amd/csrc/host/mcq_query_mpi.cpp,
which reads as the reference does (std::getline, src/sequence_io.cpp:122-285)."""
import random


def read_records(data):
    """bytes of one file -> [(header up to its first ' ', sequence, byte offset of the record)]"""
    lines, pos = [], 0
    while pos < len(data):                                   # std::getline: a last line without '\n' still counts
        e = data.find(b"\n", pos)
        e = len(data) if e < 0 else e
        lines.append((data[pos:e], pos))
        pos = e + 1
    recs, i = [], 0
    while i < len(lines):
        line, at = lines[i]
        i += 1
        if not line:
            continue
        if line[:1] == b"@":
            seq = lines[i][0] if i < len(lines) else b""
            i += 3                                           # sequence, '+', qualities (a failed getline leaves them empty)
            recs.append([line[1:], seq, at])
        elif line[:1] == b">":
            recs.append([line[1:], b"", at])
        elif recs:
            recs[-1][1] += line
    return [(h.split(b" ")[0], s, at) for h, s, at in recs]


def _seq(rng, n):
    return "".join(rng.choice("ACGTACGTACGTN") for _ in range(n))


def _fastq(rng, n, eol="\n", final=True, qual_at=False, blank=False, hdr=lambda i: "r%d desc %d" % (i, i), lens=(1, 60)):
    out = []
    for i in range(n):
        s = _seq(rng, rng.randint(*lens))
        q = ("@" if qual_at else "I") + "I" * (len(s) - 1) if s else ""
        out.append("@%s%s%s%s+%s%s%s" % (hdr(i), eol, s, eol, eol, q, eol))
        if blank and i % 3 == 1:
            out.append(eol)
    t = "".join(out)
    return (t if final else t[: -len(eol)]).encode()


def _fasta(rng, n, width=0, eol="\n", blank=False, hdr=lambda i: "r%d some description" % i, lens=(1, 200)):
    out = []
    for i in range(n):
        s = _seq(rng, rng.randint(*lens))
        body = [s] if not width else [s[k:k + width] for k in range(0, len(s), width)]
        out.append(">" + hdr(i) + eol + "".join(b + eol for b in body))
        if blank and i % 4 == 2:
            out.append(eol)
    return "".join(out).encode()


def _cut_in_last_sequence(t):
    return t[: t.rfind(b"\n+\n") - 5]                      # the file ends inside the last record's sequence line


def corpus():
    """name -> (list of file contents, strict): strict = every file is in the form the device step parses itself
    (FASTQ of 4-line records, FASTA of '>' headers and sequence lines, no empty line, one format per file)"""
    rng = random.Random(12345)
    c = {
        "fq_lf": ([_fastq(rng, 40)], True),
        "fq_crlf": ([_fastq(rng, 40, eol="\r\n")], True),
        "fq_no_final_newline": ([_fastq(rng, 40, final=False)], True),
        "fq_quality_at": ([_fastq(rng, 40, qual_at=True)], True),
        "fq_blank_lines": ([_fastq(rng, 30, blank=True)], False),
        "fa_one_line": ([_fasta(rng, 40)], True),
        "fa_wrap60": ([_fasta(rng, 30, width=60)], True),
        "fa_wrap80": ([_fasta(rng, 30, width=80)], True),
        "fa_wrap60_crlf": ([_fasta(rng, 30, width=60, eol="\r\n")], True),
        "fa_blank_lines": ([_fasta(rng, 30, width=60, blank=True)], False),
        "headers_tabs": ([_fastq(rng, 30, hdr=lambda i: ("r%d\tx y" % i) if i % 3 == 0 else ("r%d" % i if i % 3 == 1 else "r%d\tt" % i))], True),
        "fa_headers_plain": ([_fasta(rng, 30, width=70, hdr=lambda i: "q%d" % i)], True),
        "long_record_fq": ([_fastq(rng, 6, lens=(900, 1500))], True),
        "long_record_fa": ([_fasta(rng, 5, width=60, lens=(1500, 3000))], True),
        "fq_truncated": ([_cut_in_last_sequence(_fastq(rng, 20, lens=(20, 60)))], False),
        "fq_truncated_after_plus": ([_fastq(rng, 20) + b"@last\nACGT\n+\n"], False),
        "fa_then_fq": ([_fasta(rng, 10, width=60) + _fastq(rng, 10)], False),
        "junk_first": ([b"junk line\n" + _fastq(rng, 10)], False),
        "paired_fq": ([_fastq(rng, 35), _fastq(rng, 25, hdr=lambda i: "m%d" % i)], True),
        "paired_fa_fq": ([_fasta(rng, 20, width=60), _fastq(rng, 28)], True),
        "paired_short_first": ([_fastq(rng, 12), _fasta(rng, 30, width=80)], True),
    }
    return c
