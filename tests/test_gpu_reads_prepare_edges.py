"""mcq_reads_prepare (csrc/mcq_stages.hip: k_rd_count, k_rd_lines, k_rd_recs, k_rd_offsets, k_rd_copy) where the corpus of
tests/test_gpu_read_stream.py does not reach: MCQ_READS_INTERLEAVED, bytes on the edges of the 16-byte loads, the 1024-byte
waves and the 4-KiB tiles, chunks large enough for every loop and grid stride and for the three-launch scan, and degenerate
records.  The expected side is always the host parser (host.parse_chunk = mcq_reads_parse), which the host tests tie to
read_records on the same small texts; every output and the scratch carry a sentinel tail (tests/reads_device.py).  A text
labelled strict (tests/read_edge_texts.py, from the contract in include/mcq.h) must not be flagged in any chunk, so every
chunk of it is compared; a text that is not must be flagged somewhere, and its unflagged chunks are compared all the same."""
import importlib

import numpy as np
import pytest
import torch

from read_edge_texts import (EDGE_FORMATS, EDGE_OFFSETS, big_text, degenerate_corpus, edge_kinds, edge_partner, edge_text, edge_text_broken,
                             interleaved_corpus, interleaved_pairs, np_fasta, np_fastq, varied_lens)
from reads_device import _check_chunk, _device_prepare

pytestmark = pytest.mark.gpu

# constants of csrc/mcq_stages.hip
MCQ_FQ_TILE = 4096                  # bytes of text per workgroup of k_rd_count / k_rd_lines
MCQ_RD_PER_THREAD = 8
OFFSETS_PASS = 1024 * MCQ_RD_PER_THREAD     # items (sequences; interleaved: pairs) k_rd_offsets scans per pass
COPY_PASS = 2048 * 4                # queries per pass of k_rd_copy: its grid is capped at 2048 workgroups of 4 waves
RECS_PASS = 1024 * 256              # records per pass of k_rd_recs: its grid is capped at 1024 workgroups of 256 threads
MCQ_SCAN_TILE = 8192                # device_exclusive_scan: more items than this take the three-launch path

BIG_Q, BIG_B = 1 << 40, 1 << 62


@pytest.fixture(scope="module")
def mods():
    pkg = importlib.import_module("metacache-mpi_amd")
    pkg.build_host()
    return importlib.import_module("metacache-mpi_amd.engine"), importlib.import_module("metacache-mpi_amd.host"), torch.device("cuda", 0)


def _seen():
    return {"flagged": 0, "clean": 0}


def _one_chunk(mods, texts, flags, max_q=BIG_Q, max_b=BIG_B, shift=0, strict=True):
    """one chunk through the device step, compared with the host parser; a strict text must not be flagged.  Returns the
    checked info, or None for a flagged chunk"""
    eng, host, dev = mods
    seen = _seen()
    out = _check_chunk(host, eng, dev, texts, flags, max_q, max_b, seen, shift)
    if strict:
        assert seen == {"flagged": 0, "clean": 1}, (flags, max_q, max_b, shift)
    return out[0] if seen["clean"] else None


def _write(tmp_path, files):
    paths = []
    for i, data in enumerate(files):
        p = tmp_path / ("r%d.txt" % (i + 1))
        p.write_bytes(data)
        paths.append(p)
    return paths


def _batches(mods, paths, chunk, interleaved=False):
    """the file(s) through host.read_batches with the device step, checked against the host parser, as `prepare` ->
    ([(header token, [mates])], seen)"""
    eng, host, dev = mods
    seen, got = _seen(), []
    prep = lambda t, f, mq, mb: _check_chunk(host, eng, dev, t, f, mq, mb, seen)
    for texts, info, bases, seq_off, hdr, _ in host.read_batches(paths, chunk, prepare=prep, interleaved=interleaved):
        n, mates = int(info[host.READS_N]), (2 if interleaved else len(texts))
        if interleaved:
            assert int(info[host.READS_CUT2]) == 0 and int(info[host.READS_COMPLETE2]) == 0
        for q in range(n):
            seqs = [bytes(bases[int(seq_off[q * mates + m]):int(seq_off[q * mates + m + 1])]) for m in range(mates)]
            got.append((texts[0][int(hdr[2 * q]):int(hdr[2 * q + 1])], seqs))
    return got, seen


# ------------------------------------------------------------------------------------------------ A: interleaved
IL_CHUNKS = [1, 37, 97, 300, 4096, 1 << 20]


@pytest.mark.parametrize("chunk", IL_CHUNKS)
@pytest.mark.parametrize("name", sorted(interleaved_corpus()))
def test_interleaved_every_chunk_size(mods, name, chunk, tmp_path):
    """the pairs of `mini` and generated FASTQ / FASTA wrapped at 60 with an even and an odd record count, CRLF texts: every
    chunk equals the host parser, the queries read back are the records of read_records paired two by two"""
    text, strict = interleaved_corpus()[name]
    got, seen = _batches(mods, _write(tmp_path, [text]), chunk, interleaved=True)
    assert [(h, s[0], s[1]) for h, s in got] == interleaved_pairs(text), (name, chunk)
    assert seen["clean"] + seen["flagged"] > 0
    if strict:
        assert seen["flagged"] == 0, (name, chunk, seen)
    else:
        assert seen["flagged"] > 0, (name, chunk, seen)


LIMITS = [(1, 1 << 62), (3, 1 << 62), (1 << 40, 150), (4, 400), (1 << 40, 1), (7, 1000)]   # of test_device_prepare_applies_the_batch_limits


@pytest.mark.parametrize("max_q,max_b", LIMITS)
@pytest.mark.parametrize("name", ["il_generated_fastq_even", "il_generated_fastq_odd", "il_generated_fasta_even", "il_generated_fasta_odd",
                                  "il_mini_fastq_odd", "il_mini_fasta_even"])
def test_interleaved_limits_on_a_whole_file(mods, name, max_q, max_b):
    """max_queries counts pairs and max_bases the bases of both mates: info, seq_off[: 2n + 1], the bases and hdr equal the
    host parser's from an aligned and an unaligned pointer, at the end of the file and inside it"""
    eng, host, dev = mods
    text, strict = interleaved_corpus()[name]
    assert strict
    for shift in (0, 3):
        for eof in (0, host.READS_EOF1):
            info = _one_chunk(mods, [text], host.READS_INTERLEAVED | eof, max_q, max_b, shift)
            n = int(info[host.READS_N])
            assert 1 <= n <= max_q and (int(info[host.READS_BASES]) <= max_b or n == 1)
            assert int(info[host.READS_CUT2]) == 0 and int(info[host.READS_COMPLETE2]) == 0


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_interleaved_mate_boundaries(mods, fmt):
    """a chunk that ends between two mates takes neither, and the cut is in front of the first mate; an odd last record is
    a query with an empty second mate where the file ends, and waits for its mate where it does not"""
    from interleaved_texts import render
    eng, host, dev = mods
    IL = host.READS_INTERLEAVED
    recs = [(b"a", b"ACGT"), (b"a/2", b"GG"), (b"b", b"TTT"), (b"b/2", b"CCCC")]
    t = render(recs, fmt, final_newline=True)
    at_b, at_b2 = t.index(b"b\n") - 1, t.index(b"b/2") - 1
    for end in range(at_b + 1, at_b2 + 2):                   # up to the first byte of b/2: record b is complete at the most
        info = _one_chunk(mods, [t[:end]], IL)
        assert int(info[host.READS_N]) == 1 and int(info[host.READS_CUT1]) == at_b, end
    info = _one_chunk(mods, [t], IL)
    assert int(info[host.READS_N]) == 1                      # b/2 is complete only with the byte that follows it
    info = _one_chunk(mods, [t + (b"@" if fmt == "fastq" else b">")], IL)
    assert int(info[host.READS_N]) == 2 and int(info[host.READS_CUT1]) == len(t)
    odd = render(recs[:3], fmt, final_newline=True)
    info = _one_chunk(mods, [odd], IL)
    assert int(info[host.READS_N]) == 1 and int(info[host.READS_COMPLETE1]) == 1 and int(info[host.READS_CUT1]) == odd.index(b"b\n") - 1
    info, bases, seq_off, hdr, _ = _device_prepare(eng, dev, [odd], IL | host.READS_EOF1, 100, 1 << 30)
    _one_chunk(mods, [odd], IL | host.READS_EOF1, 100, 1 << 30)
    assert int(info[host.READS_N]) == 2 and int(info[host.READS_COMPLETE1]) == 2 and int(info[host.READS_CUT1]) == len(odd)
    assert seq_off[:5].tolist() == [0, 4, 6, 9, 9] and bytes(bases[:9]) == b"ACGTGGTTT"
    assert [odd[int(hdr[2 * q]):int(hdr[2 * q + 1])] for q in range(2)] == [b"a", b"b"]


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_interleaved_crlf_is_flagged_and_lf_is_not(mods, fmt):
    eng, host, dev = mods
    c = interleaved_corpus()
    flagged = lambda text, flags: int(_device_prepare(eng, dev, [text], host.READS_INTERLEAVED | flags, BIG_Q, BIG_B)[0][host.READS_STATUS]) & host.READS_NOT_STRICT
    crlf, last_cr = c["il_%s_crlf" % fmt][0], c["il_%s_last_line_cr" % fmt][0]
    for flags in (0, host.READS_EOF1):
        assert flagged(crlf, flags)
        assert not flagged(crlf.replace(b"\r\n", b"\n"), flags)
        _one_chunk(mods, [crlf.replace(b"\r\n", b"\n")], host.READS_INTERLEAVED | flags)
    assert last_cr[-1:] == b"\r" and last_cr.count(b"\r") == 1
    assert flagged(last_cr, host.READS_EOF1)                 # the last line ends in '\r' only where the text ends the file
    _one_chunk(mods, [last_cr[:-1]], host.READS_INTERLEAVED | host.READS_EOF1)


# ------------------------------------------------------------------------------------------------ B: load, wave and tile edges
@pytest.mark.parametrize("fmt,kind", [(f, k) for f in EDGE_FORMATS for k in edge_kinds(f)])
def test_a_byte_on_every_load_wave_and_tile_edge(mods, fmt, kind):
    """a newline that ends a header or a sequence line, a record start, a '+', the last byte of a text with and without a
    final newline, on byte 15 / 16 / 17 (16-byte load), 1023 / 1024 / 1025 (wave), 4095 / 4096 / 4097, 8191 / 8192 (tile):
    from pointers shifted by 0, 1, 3 and 15 bytes (aligned 16-byte loads and the byte loop of rd_masks), alone and beside
    a text of another length in either place"""
    eng, host, dev = mods
    partner = edge_partner(fmt)
    both = host.READS_EOF1 | host.READS_EOF2
    for off in EDGE_OFFSETS:
        text = edge_text(fmt, kind, off)
        assert len(text) != len(partner)
        for shift in (0, 1, 3, 15):
            for flags in (0, host.READS_EOF1):
                _one_chunk(mods, [text], flags, shift=shift)
            info = _one_chunk(mods, [text, partner], both, shift=shift)
            assert int(info[host.READS_N]) >= 1
            _one_chunk(mods, [partner, text], both, shift=shift)


@pytest.mark.parametrize("fmt,kind", [(f, k) for f in EDGE_FORMATS for k in edge_kinds(f) if k in ("record_start", "plus")])
def test_a_wrong_line_start_on_every_edge_is_flagged(mods, fmt, kind):
    """the same texts with the '@' / '+' on the edge replaced by 'X' (FASTQ), the '>' by '@' (FASTA): the line start that
    the strict form prescribes is the first byte of a load, a wave or a tile, and `prev` of rd_masks comes from the byte in
    front of it; the chunk must be flagged from every pointer shift, inside the file and at its end"""
    eng, host, dev = mods
    for off in EDGE_OFFSETS:
        text = edge_text_broken(fmt, kind, off)
        for shift in (0, 1, 3, 15):
            for flags in (0, host.READS_EOF1):
                assert _one_chunk(mods, [text], flags, shift=shift, strict=False) is None, (off, shift, flags)


# ------------------------------------------------------------------------------------------------ C: launch strides, the long scan
def _cut_limits(lens_per_query, pass_queries):
    """(max_queries, max_bases) with the cut inside the first pass, exactly at its end (query pass_queries is the last
    taken), in a later pass; max_queries at the pass sizes; no limit"""
    cum = np.cumsum(lens_per_query)
    nq = len(cum)
    assert nq > pass_queries
    later = min(nq - 1, pass_queries + 1500)
    lim = [(BIG_Q, int(cum[3001]) - 1, 3001), (BIG_Q, int(cum[pass_queries - 1]), pass_queries), (BIG_Q, int(cum[later]) - 1, later)]
    lim += [(mq, BIG_B, min(mq, nq)) for mq in (4096, 4097, 8192, 8193)] + [(BIG_Q, BIG_B, nq)]
    return lim


@pytest.mark.parametrize("n", [8193, 20000])
def test_single_fastq_beyond_one_pass(mods, n):
    """more queries than one pass of k_rd_copy and of k_rd_offsets takes: the carry of the scan, the maxima across
    passes and the grid stride of the copy"""
    eng, host, dev = mods
    assert n > COPY_PASS and n > OFFSETS_PASS
    lens = varied_lens(n, 5)
    text = np_fastq(lens, seed=n)
    for max_q, max_b, want in _cut_limits(lens, OFFSETS_PASS):
        info = _one_chunk(mods, [text], host.READS_EOF1, max_q, max_b)
        assert int(info[host.READS_N]) == want, (max_q, max_b)


@pytest.mark.parametrize("n", [4097, 12000])
def test_two_fastq_texts_beyond_one_pass(mods, n):
    """two texts: the scan runs over ns = 2 n sequences, which crosses its pass at pair 4096"""
    eng, host, dev = mods
    assert 2 * n > OFFSETS_PASS
    l1, l2 = varied_lens(n, 6), varied_lens(n + 5, 7)
    t1, t2 = np_fastq(l1, seed=n), np_fastq(l2, seed=n + 1)
    for max_q, max_b, want in _cut_limits(l1 + l2[:n], OFFSETS_PASS // 2):
        info = _one_chunk(mods, [t1, t2], host.READS_EOF1 | host.READS_EOF2, max_q, max_b)
        assert int(info[host.READS_N]) == want, (max_q, max_b)


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_interleaved_beyond_one_pass(mods, fmt):
    """8193 pairs (and a last record without a mate): one length per pair, seq_off written with a stride of 2"""
    eng, host, dev = mods
    n = 8193
    assert n > COPY_PASS and n > OFFSETS_PASS
    lens = varied_lens(2 * n + 1, 8, 1, 150)
    text = np_fastq(lens, seed=3) if fmt == "fastq" else np_fasta(lens, width=60, seed=3)
    pair = np.add.reduceat(lens, np.arange(0, len(lens), 2))
    assert len(pair) == n + 1
    for max_q, max_b, want in _cut_limits(pair, OFFSETS_PASS):
        info = _one_chunk(mods, [text], host.READS_INTERLEAVED | host.READS_EOF1, max_q, max_b)
        assert int(info[host.READS_N]) == want, (max_q, max_b)
    info = _one_chunk(mods, [text], host.READS_INTERLEAVED)             # inside the file the last record waits for its mate
    assert int(info[host.READS_N]) == n


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_minimal_records_beyond_the_grid_of_k_rd_recs(mods, fmt):
    """262 145 + 1000 records of 8 bytes ("@\\nA\\n+\\nI\\n") or 4 bytes (">\\nA\\n"), a few of them longer: one thread per
    record no longer covers them, and a FASTA text has one header every 4 bytes (the header count path, X.hl)"""
    eng, host, dev = mods
    n = RECS_PASS + 1 + 1000
    lens = np.ones(n, np.int64)
    lens[1::997] = varied_lens(len(lens[1::997]), 9, 2, 50)
    text = np_fastq(lens, name_width=0, seed=4) if fmt == "fastq" else np_fasta(lens, name_width=0, seed=4)
    if fmt == "fastq":
        assert len(text[:8]) == 8 and (text[0:2], text[3:6], text[7:9]) == (b"@\n", b"\n+\n", b"\n@")
    else:
        assert (text[0:2], text[3:6]) == (b">\n", b"\n>\n")
    assert len(text) == (8 if fmt == "fastq" else 4) * n + (2 if fmt == "fastq" else 1) * int((lens - 1).sum())
    for flags, want in ((host.READS_EOF1, n), (0, n - 1)):
        info = _one_chunk(mods, [text], flags)
        assert int(info[host.READS_N]) == want > RECS_PASS


@pytest.mark.parametrize("shift", [0, 5])
@pytest.mark.parametrize("fmt", ["fastq", "fasta_wrapped"])
def test_text_above_32_mib_takes_the_three_launch_scan(mods, fmt, shift):
    """more than 8192 tiles: the scans of the newline counts and of the header counts run as tile scan, scan of the tile
    sums and add; long records keep the host side short"""
    eng, host, dev = mods
    text, n = big_text(fmt)
    assert (len(text) + MCQ_FQ_TILE - 1) // MCQ_FQ_TILE > MCQ_SCAN_TILE
    info = _one_chunk(mods, [text], host.READS_EOF1, shift=shift)
    assert int(info[host.READS_N]) == n and int(info[host.READS_CUT1]) == len(text)


# ------------------------------------------------------------------------------------------------ D: degenerate records
@pytest.mark.parametrize("name", sorted(degenerate_corpus()))
def test_degenerate_records(mods, name, tmp_path):
    """empty sequence lines, headers in a row, empty headers, a header that starts with ' ' or ends the text, texts of 0
    and 1 bytes, a "\\r" line: chunks of 1, 37 and 2^20 bytes and the whole text as one chunk, inside the file and at its end"""
    from read_corpus import read_records
    eng, host, dev = mods
    files, strict = degenerate_corpus()[name]
    recs = [read_records(f) for f in files]
    exp = [(recs[0][q][0], [r[q][1] for r in recs]) for q in range(min(len(r) for r in recs))]
    paths = _write(tmp_path, files)
    for chunk in (1, 37, 1 << 20):
        got, seen = _batches(mods, paths, chunk)
        assert got == exp, (name, chunk)
        assert seen["clean"] + seen["flagged"] > 0
        if strict:
            assert seen["flagged"] == 0, (name, chunk, seen)
        else:
            assert seen["flagged"] > 0, (name, chunk, seen)
    both = host.READS_EOF1 | (host.READS_EOF2 if len(files) > 1 else 0)
    for flags in (0, both):
        for shift in (0, 3):
            info = _one_chunk(mods, files, flags, shift=shift, strict=strict)
            if flags and not strict:
                assert info is None, name                    # the whole file is there: what is not strict in it is seen
            if flags and strict:
                assert int(info[host.READS_N]) == len(exp), name
