"""mcq_reads_prepare with MCQ_READS_INTERLEAVED (records 2q, 2q+1 of one text are the mates of query q) against the host
parser with the same flag, which tests/test_host_reads_interleaved.py checks against the two-file parse: queries, seq_off,
bases, header ranges, cut point and complete counts, with the chunk cut at every byte across a record boundary and a pair
boundary, with and without MCQ_READS_EOF1, and from unaligned text."""
import importlib

import numpy as np
import pytest
import torch

from interleaved_texts import interleaved_records, render

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    pkg = importlib.import_module("metacache-mpi_amd")
    pkg.build_host()
    return importlib.import_module("metacache-mpi_amd.engine"), importlib.import_module("metacache-mpi_amd.host")


def _device(eng, text, flags, max_q, max_b, shift=0):
    """mcq_reads_prepare on one interleaved chunk -> (info, bases, seq_off, hdr, qcap) as numpy arrays"""
    dev = torch.device("cuda", 0)
    L = len(text)
    qcap = max(1, min(max_q, L // 2 + 2))
    buf = torch.zeros(L + shift + 1, dtype=torch.uint8, device=dev)
    if L:
        buf[shift:shift + L] = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to(dev)
    sb = eng.reads_scratch_bytes(L, 0, qcap)
    scratch = torch.empty(sb, dtype=torch.uint8, device=dev)
    bases = torch.zeros(L + 1, dtype=torch.uint8, device=dev)
    seq_off = torch.zeros(2 * qcap + 1, dtype=torch.int64, device=dev)
    hdr = torch.zeros(2 * qcap, dtype=torch.int64, device=dev)
    info = torch.full((eng.MCQ_READS_INFO_WORDS,), 7, dtype=torch.int64, device=dev)
    eng.reads_prepare(buf.data_ptr() + shift, L, None, 0, flags | eng.MCQ_READS_INTERLEAVED, qcap, max_b, scratch.data_ptr(), sb,
                      bases.data_ptr(), seq_off.data_ptr(), hdr.data_ptr(), info.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    return (info.cpu().numpy().view(np.uint64), bases.cpu().numpy(), seq_off.cpu().numpy().view(np.uint64),
            hdr.cpu().numpy().view(np.uint64), qcap)


def _check(eng, host, text, flags, max_q=1 << 40, max_b=1 << 62, shift=0):
    """the device step equals the host parser unless it flags the chunk; returns the host's info, and whether it was flagged"""
    info, bases, seq_off, hdr, qcap = _device(eng, text, flags, max_q, max_b, shift)
    hinfo, hbases, hseq_off, hhdr = host.parse_chunk([text], flags | host.READS_INTERLEAVED, qcap, max_b)
    if int(info[host.READS_STATUS]) & host.READS_NOT_STRICT:
        return hinfo, True
    n, nb = int(hinfo[host.READS_N]), int(hinfo[host.READS_BASES])
    assert info.tolist() == hinfo.tolist(), (len(text), flags, info.tolist(), hinfo.tolist())
    assert seq_off[: 2 * n + 1].tolist() == hseq_off[: 2 * n + 1].tolist()
    assert bytes(bases[:nb]) == bytes(hbases[:nb])
    assert hdr[: 2 * n].tolist() == hhdr[: 2 * n].tolist()
    return hinfo, False


def _small(fmt, odd=True):
    """a few records: five pairs of `mini` cut to at most 70 bases (FASTA lines wrap at 60), and a record without a mate"""
    recs = [(h, s[:30 + 10 * (i % 5)]) for i, (h, s) in enumerate(interleaved_records(odd=False)[:10])]
    if odd:
        recs.append((b"lonely read", b"ACGTTGCA"))
    return recs, render(recs, fmt, final_newline=True)


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_cut_at_every_byte_across_a_record_and_a_pair_boundary(mods, fmt):
    """the chunk ends at every byte from the header of record 2 to the sequence of record 5: between the mates of query 1,
    between queries 1 and 2, and inside both; as a chunk of a longer file and as the end of one.  A chunk that ends
    between two mates takes neither"""
    eng, host = mods
    recs, text = _small(fmt)
    mark = b"@" if fmt == "fastq" else b">"
    start = [text.index(mark + h + b"\n") for h, _ in recs]
    ends = 0
    for end in range(start[2], start[5] + len(recs[5][0]) + 12):
        for flags in (0, host.READS_EOF1):
            hinfo, flagged = _check(eng, host, text[:end], flags)
            ends += 1
            assert not flagged or (flags and fmt == "fastq"), (end, flags)      # only a FASTQ file that ends inside a record is not strict
            if flags == 0:      # records complete in text[:end]: those whose successor has begun
                complete = sum(1 for s in start[1:] if s < end)
                assert int(hinfo[host.READS_N]) == complete // 2, end
                assert int(hinfo[host.READS_CUT1]) == start[2 * (complete // 2)], end
            else:
                assert flagged or int(hinfo[host.READS_CUT1]) == end
    assert ends > 2 * (start[5] - start[2])


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
@pytest.mark.parametrize("odd", [False, True])
def test_whole_fixture_coarse_cuts_and_unaligned_text(mods, fmt, odd):
    """the 197 pairs of `mini` (several tiles of text, 2 kb reads, an N read, a lowercase read), no final newline: the whole
    text and the chunks text[:end] at a coarse set of ends, from aligned and unaligned pointers; the odd record at the end
    is a query with an empty second mate"""
    eng, host = mods
    recs = interleaved_records(odd=odd)
    text = render(recs, fmt, final_newline=False)
    hinfo, flagged = _check(eng, host, text, host.READS_EOF1)
    assert not flagged and int(hinfo[host.READS_N]) == (len(recs) + 1) // 2 and int(hinfo[host.READS_CUT1]) == len(text)
    hinfo, flagged = _check(eng, host, text, 0)
    assert not flagged and int(hinfo[host.READS_N]) == (len(recs) - 1) // 2
    for end in list(range(1, len(text), 4099)) + [4096, 8192]:
        for shift in (0, 3):
            _, flagged = _check(eng, host, text[:end], 0, shift=shift)
            assert not flagged
            _check(eng, host, text[:end], host.READS_EOF1, shift=shift)


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
@pytest.mark.parametrize("max_q,max_b", [(1, 1 << 62), (2, 1 << 62), (3, 1 << 62), (1 << 40, 20), (4, 400), (1 << 40, 5000)])
def test_limits_count_pairs(mods, fmt, max_q, max_b):
    """max_queries counts pairs, max_bases the bases of both mates; a first pair larger than max_bases goes alone"""
    eng, host = mods
    text = render(interleaved_records(odd=True)[:81], fmt, final_newline=True)
    for flags in (0, host.READS_EOF1):
        hinfo, flagged = _check(eng, host, text, flags, max_q, max_b)
        n = int(hinfo[host.READS_N])
        assert not flagged and 1 <= n <= max_q and (int(hinfo[host.READS_BASES]) <= max_b or n == 1)


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_crlf_text_goes_to_the_host(mods, fmt):
    eng, host = mods
    recs, _ = _small(fmt)
    text = render(recs, fmt, final_newline=True, eol=b"\r\n")
    for flags in (0, host.READS_EOF1):
        info = _device(eng, text, flags, 1 << 40, 1 << 62)[0]
        assert int(info[host.READS_STATUS]) & host.READS_NOT_STRICT
    info = _device(eng, text[:-1], host.READS_EOF1, 1 << 40, 1 << 62)[0]       # ... and a file that ends in the '\r'
    assert int(info[host.READS_STATUS]) & host.READS_NOT_STRICT
    lone = render(recs, fmt, final_newline=True)[:-1] + b"\r"                # LF text whose last line alone ends in one
    info = _device(eng, lone, host.READS_EOF1, 1 << 40, 1 << 62)[0]
    assert int(info[host.READS_STATUS]) & host.READS_NOT_STRICT


def test_the_flag_is_refused_with_a_second_text(mods):
    eng, host = mods
    dev = torch.device("cuda", 0)
    t = torch.zeros(64, dtype=torch.uint8, device=dev)
    sb = eng.reads_scratch_bytes(8, 8, 4)
    scratch = torch.zeros(sb, dtype=torch.uint8, device=dev)
    with pytest.raises(Exception, match="INTERLEAVED"):
        eng.reads_prepare(t.data_ptr(), 8, t.data_ptr(), 8, eng.MCQ_READS_INTERLEAVED, 4, 100, scratch.data_ptr(), sb, t.data_ptr(), t.data_ptr(),
                          t.data_ptr(), t.data_ptr(), 0)
