"""mcq_reads_prepare on one chunk per file, for the GPU tests (tests/test_gpu_read_stream.py,
tests/test_gpu_reads_prepare_edges.py): every output and the scratch get a sentinel tail behind the capacity that
include/mcq.h states, the tails are checked after the call, and the result is compared with the host parser
(mcq_reads_parse) in numpy."""
import numpy as np
import torch

SENT8 = 0x5A
SENT64 = 0x5A5A5A5A5A5A5A5A
TAIL = 64                   # bytes behind bases and the scratch, words behind seq_off, hdr and info


def _dev_bytes(data, dev, shift=0):
    buf = torch.zeros(len(data) + shift + 1, dtype=torch.uint8, device=dev)
    if len(data):
        buf[shift:shift + len(data)] = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(dev)
    return buf


def _guarded(n, dtype, dev, fill=None):
    """n elements (zeros, or `fill`) and a tail of sentinels"""
    sent = SENT8 if dtype == torch.uint8 else SENT64
    t = torch.full((n + TAIL,), sent, dtype=dtype, device=dev)
    t[:n] = 0 if fill is None else fill
    return t


def _down(t, n, what):
    """the first n elements as a numpy array, after checking that the tail was left alone"""
    sent = SENT8 if t.dtype == torch.uint8 else SENT64
    assert bool((t[n:] == sent).all()), "%s: written behind its capacity of %d" % (what, n)
    a = t[:n].cpu().numpy()
    return a if t.dtype == torch.uint8 else a.view(np.uint64)


def _device_prepare(eng, dev, texts, flags, max_q, max_b, shift=0):
    """mcq_reads_prepare on one chunk per file -> (info, bases, seq_off, hdr, qcap) as numpy arrays.  Capacities as the
    contract states them: bases len1 + len2, seq_off 2 * max_queries + 1, hdr 2 * max_queries, info MCQ_READS_INFO_WORDS,
    the scratch mcq_reads_scratch_bytes; nothing may be written behind any of them"""
    L = [len(t) for t in texts]
    qcap = max(1, min(max_q, min(L) // 2 + 2))
    bufs = [_dev_bytes(t, dev, shift) for t in texts]
    ptr = [b.data_ptr() + shift for b in bufs]
    L2 = L[1] if len(texts) > 1 else 0
    sb = eng.reads_scratch_bytes(L[0], L2, qcap)
    scratch = _guarded(sb, torch.uint8, dev)
    bases = _guarded(L[0] + L2, torch.uint8, dev)
    seq_off = _guarded(2 * qcap + 1, torch.int64, dev)
    hdr = _guarded(2 * qcap, torch.int64, dev)
    info = _guarded(eng.MCQ_READS_INFO_WORDS, torch.int64, dev, fill=7)
    eng.reads_prepare(ptr[0], L[0], ptr[1] if len(texts) > 1 else None, L2, flags, qcap, max_b, scratch.data_ptr(), sb,
                      bases.data_ptr(), seq_off.data_ptr(), hdr.data_ptr(), info.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    assert bool((scratch[sb:] == SENT8).all()), "scratch: written behind mcq_reads_scratch_bytes = %d" % sb
    return (_down(info, eng.MCQ_READS_INFO_WORDS, "info"), _down(bases, L[0] + L2, "bases"),
            _down(seq_off, 2 * qcap + 1, "seq_off"), _down(hdr, 2 * qcap, "hdr"), qcap)


def _check_chunk(host, eng, dev, texts, flags, max_q, max_b, seen, shift=0):
    """the device step on one chunk; equal to the host parser unless it flags the chunk.  Returns what the CLI uses.
    flags may hold READS_INTERLEAVED (one text; the outputs then have the paired form)"""
    info, bases, seq_off, hdr, qcap = _device_prepare(eng, dev, texts, flags, max_q, max_b, shift)
    h = host.parse_chunk(texts, flags, qcap, max_b)
    if int(info[host.READS_STATUS]) & host.READS_NOT_STRICT:
        seen["flagged"] += 1
        return h
    seen["clean"] += 1
    hinfo, hbases, hseq_off, hhdr = h
    n, mates = int(hinfo[host.READS_N]), (2 if flags & host.READS_INTERLEAVED else len(texts))
    assert np.array_equal(info, hinfo), (info.tolist(), hinfo.tolist())
    assert np.array_equal(seq_off[: n * mates + 1], hseq_off[: n * mates + 1])
    nb = int(hinfo[host.READS_BASES])
    assert np.array_equal(bases[:nb], hbases[:nb])
    assert np.array_equal(hdr[: 2 * n], hhdr[: 2 * n])
    return info, bases, seq_off, hdr
