"""Read texts built for the edges of mcq_reads_prepare's kernels (tests/test_gpu_reads_prepare_edges.py, tests/test_gpu_fastq.py)
and, the small ones, for the host parser's tests (tests/test_host_read_stream.py, tests/test_host_reads_interleaved.py):
a chosen byte on a chosen offset (16-byte loads, 1024-byte waves, 4096-byte tiles), degenerate records, and large texts
made with numpy.  Every text carries a `strict` label, written from the contract of mcq_reads_prepare in include/mcq.h:
FASTQ of 4-line records (line 1 '@', line 3 '+'), or FASTA of '>' header lines and non-empty sequence lines, one format
per text; a record may have an empty header, an empty sequence line (FASTQ) or no sequence line at all (FASTA)."""
import functools
import random

import numpy as np

from read_corpus import _fasta, _fastq, read_records

# ---------------------------------------------------------------------------------------------------------------- B
EDGE_OFFSETS = [15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192]
EDGE_FORMATS = ["fastq", "fasta_one_line", "fasta_wrapped"]
EDGE_KINDS = ["header_newline", "sequence_newline", "record_start", "plus", "last_newline", "last_byte"]

_TAIL_SEQS = ["ACGTTGCAAC" * 7 + "GGT", "TTGACC", "N" * 61 + "ACGT" * 20, "GATTACA" * 9]


def _record(fmt, name, seq, width=60):
    if fmt == "fastq":
        return "@%s\n%s\n+\n%s\n" % (name, seq, "I" * len(seq))
    if fmt == "fasta_one_line":
        return ">%s\n%s\n" % (name, seq)
    return ">%s\n%s" % (name, "".join(seq[k:k + width] + "\n" for k in range(0, len(seq), width)))


def edge_kinds(fmt):
    return [k for k in EDGE_KINDS if k != "plus" or fmt == "fastq"]


def edge_text(fmt, kind, off):
    """a strict text whose first header is padded so that the byte `kind` names lies at byte offset off; the place is
    asserted here, so a change of the generator cannot move the byte off the edge unnoticed"""
    def build(pad, tail):
        name = "r0" + (" " + "p" * (pad - 1) if pad else "")           # (pad 0: a header without a ' ')
        first = _record(fmt, name, seq0, width=3)                       # (wrapped: lines ACG, TAC, G)
        return (first + "".join(_record(fmt, "t%d tail" % i, s) for i, s in enumerate(_TAIL_SEQS[:tail]))).encode()

    def place(text):
        nl = [i for i in range(len(text)) if text[i:i + 1] == b"\n"]
        if kind == "header_newline":
            return nl[0]
        if kind == "sequence_newline":
            return nl[1]
        if kind == "record_start":
            return read_records(text)[1][2]
        if kind == "plus":
            return nl[1] + 1
        return len(text) - 1
    tail, seq0 = 4, "ACGTACG"
    if off < 1000 and kind in ("record_start", "last_newline", "last_byte"):
        seq0 = "AG"                                                     # (a whole record in front of byte 15)
        tail = 4 if kind == "record_start" else 0
    cut = 1 if kind == "last_byte" else 0
    base = build(0, tail)
    pad = off - place(base[:len(base) - cut])
    assert pad >= 0, (fmt, kind, off)
    text = build(pad, tail)
    text = text[:len(text) - cut]
    want = {"header_newline": b"\n", "sequence_newline": b"\n", "record_start": b"@" if fmt == "fastq" else b">", "plus": b"+",
            "last_newline": b"\n"}.get(kind)
    assert place(text) == off and (want is None or text[off:off + 1] == want), (fmt, kind, off)
    if kind == "header_newline":
        assert text.index(b"\n") == off
    elif kind == "sequence_newline":
        assert text[off - 1:off] in (b"G", b"g") and text.count(b"\n", 0, off) == 1
    elif kind == "record_start":
        assert text[off - 1:off] == b"\n" and text[off:off + 3] in (b"@t0", b">t0")
    elif kind == "plus":
        assert text[off - 1:off + 2] == b"\n+\n"
    elif kind == "last_newline":
        assert len(text) == off + 1 and text[-1:] == b"\n"
    else:
        assert len(text) == off + 1 and text[-1:] not in (b"\n", b"")
    return text


def edge_text_broken(fmt, kind, off):
    """edge_text with the byte on the edge replaced, for the two kinds that are line starts the strict form prescribes: a
    FASTQ record that starts with 'X' or whose third line does; a FASTA text with a line that starts with '@'.  Not strict"""
    assert kind in ("record_start", "plus")
    text = edge_text(fmt, kind, off)
    broken = text[:off] + (b"X" if fmt == "fastq" else b"@") + text[off + 1:]
    assert len(broken) == len(text) and broken[off - 1:off] == b"\n" and broken != text
    return broken


def edge_partner(fmt):
    """a second text of another length for the two-text runs: a few hundred bytes, so it is the longer text at the small
    offsets and the shorter one (its grid row returns early) at the large ones"""
    rng = random.Random(77)
    return _fastq(rng, 6, lens=(20, 60)) if fmt == "fastq" else _fasta(rng, 6, width=0 if fmt == "fasta_one_line" else 60, lens=(20, 150))


def edge_corpus():
    """name -> ([text], strict) of every text of part B, in the form of read_corpus.corpus()"""
    c = {"edge_%s_%s_%d" % (fmt, kind, off): ([edge_text(fmt, kind, off)], True)
         for fmt in EDGE_FORMATS for kind in edge_kinds(fmt) for off in EDGE_OFFSETS}
    c.update({"edge_%s_broken-%s_%d" % (fmt, kind, off): ([edge_text_broken(fmt, kind, off)], False)
              for fmt in EDGE_FORMATS for kind in edge_kinds(fmt) if kind in ("record_start", "plus") for off in EDGE_OFFSETS})
    return c


# ---------------------------------------------------------------------------------------------------------------- D
def degenerate_corpus():
    """name -> (texts, strict): degenerate records, each alone and inside a longer file"""
    rng = random.Random(4711)
    fq_a, fq_b = _fastq(rng, 5, lens=(1, 70)), _fastq(rng, 4, lens=(1, 70), hdr=lambda i: "z%d" % i)
    fa_a, fa_b = _fasta(rng, 5, width=60, lens=(1, 150)), _fasta(rng, 4, width=60, lens=(1, 150), hdr=lambda i: "z%d" % i)
    c = {}

    def both(name, fmt, text, strict, inside_strict=None):
        a, b = (fq_a, fq_b) if fmt == "fq" else (fa_a, fa_b)
        c[name + "_alone"] = ([text], strict)
        c[name + "_inside"] = ([a + text + b], strict if inside_strict is None else inside_strict)

    # FASTQ: 4-line records whose lines 2 and 4 are empty are strict (line 1 '@', line 3 '+')
    both("fq_empty_sequence", "fq", b"@e d\n\n+\n\n", True)
    both("fq_empty_header", "fq", b"@\nACGT\n+\nIIII\n", True)
    both("fq_header_starts_with_space", "fq", b"@ x y\nACGT\n+\nIIII\n", True)
    both("fq_one_record", "fq", b"@a x\nACGT\n+\nIIII\n", True)
    c["fq_one_record_no_final_newline"] = ([b"@a x\nACGT\n+\nIIII"], True)
    c["fq_minimal_records"] = ([b"@\nA\n+\nI\n" * 7], True)
    # a FASTQ file that ends inside a record is not strict: its last record has fewer than 4 lines
    c["fq_header_ends_the_text_alone"] = ([b"@abc"], False)
    c["fq_header_ends_the_text_inside"] = ([fq_a + b"@abc"], False)
    c["fq_single_at"] = ([b"@"], False)
    # FASTA: a header followed by the next header, or by the end of the text, is a record without a sequence line; every
    # sequence line that is there is non-empty: strict
    both("fa_two_headers_first", "fa", b">a d\n>b\nAC\n>c\nGT\n", True)
    both("fa_two_headers_middle", "fa", b">a\nAC\n>b d\n>c\nGT\n", True)
    both("fa_two_headers_last", "fa", b">a\nAC\n>b\nGT\n>c d\n", True)
    c["fa_only_headers"] = ([b">a\n>b\n>c"], True)
    both("fa_empty_header", "fa", b">\nACGT\n", True)
    both("fa_header_starts_with_space", "fa", b"> x y\nACGT\n", True)
    both("fa_one_record", "fa", b">a x\nACGT\nTTG\n", True)
    c["fa_header_ends_the_text_alone"] = ([b">abc"], True)
    c["fa_header_ends_the_text_inside"] = ([fa_a + b">abc"], True)
    c["fa_single_gt"] = ([b">"], True)
    c["fa_minimal_records"] = ([b">\nA\n" * 9], True)
    # a line that is only "\r" is a non-empty sequence line (getline keeps the '\r')
    both("fa_cr_only_line", "fa", b">a\nAC\n\r\nGT\n", True)
    # two texts, one of length 0: no query, nothing to flag
    c["empty_text_first"] = ([b"", fq_a], True)
    c["empty_text_second"] = ([fa_a, b""], True)
    c["empty_text_alone"] = ([b""], True)
    return c


# ---------------------------------------------------------------------------------------------------------------- A
def interleaved_corpus():
    """name -> (text, strict) for MCQ_READS_INTERLEAVED: records 2q, 2q+1 are the mates of query q.  Strict as above, and no
    line may end in '\\r'"""
    from interleaved_texts import interleaved_records, render
    rng = random.Random(2024)
    c = {}
    for odd in (False, True):
        tag = "odd" if odd else "even"
        for fmt in ("fastq", "fasta"):
            c["il_mini_%s_%s" % (fmt, tag)] = (render(interleaved_records(odd=odd), fmt, final_newline=False), True)
        c["il_generated_fastq_%s" % tag] = (_fastq(rng, 30 + odd), True)
        c["il_generated_fasta_%s" % tag] = (_fasta(rng, 30 + odd, width=60), True)
    c["il_fastq_crlf"] = (_fastq(rng, 12, eol="\r\n"), False)
    c["il_fasta_crlf"] = (_fasta(rng, 12, width=60, eol="\r\n"), False)
    c["il_fastq_last_line_cr"] = (_fastq(rng, 12, final=False) + b"\r", False)
    c["il_fasta_last_line_cr"] = (_fasta(rng, 12, width=60)[:-1] + b"\r", False)
    return c


def interleaved_pairs(text):
    """[(header token, mate 0, mate 1)] as read_records and sequence_pair_reader::next pair them: an odd last record is a
    query with an empty second mate"""
    r = read_records(text)
    return [(r[i][0], r[i][1], r[i + 1][1] if i + 1 < len(r) else b"") for i in range(0, len(r), 2)]


# ---------------------------------------------------------------------------------------------------------------- C
_LUT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _put_names(buf, start, name_width):
    """the decimal record number, name_width digits, behind the byte at start"""
    idx = np.arange(len(start), dtype=np.int64)
    for k in range(name_width):
        buf[start + 1 + k] = (48 + (idx // 10 ** (name_width - 1 - k)) % 10).astype(np.uint8)


def np_fastq(lens, name_width=7, seed=1):
    """FASTQ text of records "@<number>\\n<bases>\\n+\\n<qualities>\\n" with these sequence lengths, as bytes; the bases and
    the quality characters are random letters of ACGT (any byte but a newline is a quality)"""
    lens = np.asarray(lens, dtype=np.int64)
    size = 1 + name_width + 1 + lens + 1 + 2 + lens + 1
    start = np.concatenate([[0], np.cumsum(size)[:-1]]).astype(np.int64)
    buf = _LUT[np.random.default_rng(seed).integers(0, 4, size=int(size.sum()), dtype=np.uint8)]
    buf[start] = ord("@")
    _put_names(buf, start, name_width)
    hn = start + 1 + name_width
    buf[hn] = 10
    buf[hn + 1 + lens] = 10
    buf[hn + 2 + lens] = ord("+")
    buf[hn + 3 + lens] = 10
    buf[hn + 4 + 2 * lens] = 10
    return buf.tobytes()


def np_fasta(lens, name_width=7, width=0, seed=2):
    """FASTA text of records "><number>\\n" + the bases on one line (width 0) or wrapped at `width` columns, as bytes"""
    lens = np.asarray(lens, dtype=np.int64)
    assert lens.min() >= 1
    nlines = np.ones(len(lens), np.int64) if not width else (lens + width - 1) // width
    size = 1 + name_width + 1 + lens + nlines
    start = np.concatenate([[0], np.cumsum(size)[:-1]]).astype(np.int64)
    buf = _LUT[np.random.default_rng(seed).integers(0, 4, size=int(size.sum()), dtype=np.uint8)]
    buf[start] = ord(">")
    _put_names(buf, start, name_width)
    s0 = start + 1 + name_width
    buf[s0] = 10
    buf[start + size - 1] = 10                                          # the newline of the last line
    if width:
        rec = np.repeat(np.arange(len(lens)), nlines - 1)               # the full lines in front of it
        first = np.concatenate([[0], np.cumsum(nlines - 1)[:-1]])
        k = np.arange(len(rec)) - first[rec]
        buf[s0[rec] + (k + 1) * (width + 1)] = 10
    return buf.tobytes()


def varied_lens(n, seed, lo=1, hi=60):
    return np.random.default_rng(seed).integers(lo, hi + 1, size=n)


@functools.lru_cache(maxsize=None)
def big_text(fmt):
    """a text above 32 MiB (more than 8192 tiles of 4 KiB) of long records, 2 to 5 kb each: "fastq", "fasta_wrapped" (60
    columns) or "fasta_one_line" -> (bytes, number of records)"""
    lens = varied_lens(5200 if fmt == "fastq" else 10400, 99, 2000, 5000)
    if fmt == "fastq":
        return np_fastq(lens, seed=11), len(lens)
    return np_fasta(lens, width=60 if fmt == "fasta_wrapped" else 0, seed=12), len(lens)
