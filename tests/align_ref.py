"""A plain restatement of what the reference computes for `-align`: align_semi_global with default_alignment_scheme
(src/alignment.h) and make_semi_global_alignment (src/classification.cpp:77-103).  The score matrix is filled one anti-diagonal
at a time (numpy), everything else follows the reference's loops.  tests/test_align_ref.py holds it to the recorded cases."""
import numpy as np

MATCH, MISMATCH, GAP = 2, -1, -1
_RC = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def reverse_complement(seq):
    """reverse_complement of src/dna_encoding.h:146-165: only ACGTacgt change"""
    return bytes(seq)[::-1].translate(_RC)


def _first_greater(values, best):
    """the reference's `if (value > best)` loop over `values` in ascending order: index of the element it ends on, or -1"""
    if len(values) == 0:
        return -1
    m = int(values.max())
    return int(np.argmax(values)) if m > best else -1


def align_semi_global(query, subject, backtrace=True):
    """(score, aligned query, aligned subject); the two strings are b"" for backtrace=False"""
    q = np.frombuffer(bytes(query), np.uint8)
    s = np.frombuffer(bytes(subject), np.uint8)
    lq, ls = len(q), len(s)
    H = np.zeros((lq + 1, ls + 1), np.int32)
    P = np.zeros((lq + 1, ls + 1), np.uint8)               # 0 none, 1 diag, 2 above, 3 left
    for d in range(2, lq + ls + 1):
        i = np.arange(max(1, d - ls), min(lq, d - 1) + 1)
        j = d - i
        sc = H[i - 1, j - 1] + np.where(q[i - 1] == s[j - 1], MATCH, MISMATCH)
        pr = np.ones(len(i), np.uint8)
        a = H[i - 1, j] + GAP
        m = a > sc
        sc = np.where(m, a, sc); pr[m] = 2
        l = H[i, j - 1] + GAP
        m = l > sc
        sc = np.where(m, l, sc); pr[m] = 3
        H[i, j] = sc
        P[i, j] = pr
    bq, bs, bv = lq, ls, int(H[lq, ls])
    k = _first_greater(H[1:lq, ls], bv) if lq > 1 else -1
    if k >= 0:
        bq, bs, bv = k + 1, ls, int(H[k + 1, ls])
    k = _first_greater(H[lq, 1:ls], bv) if ls > 1 else -1
    if k >= 0:
        bq, bs, bv = lq, k + 1, int(H[lq, k + 1])
    if not backtrace:
        return bv, b"", b""
    aq, asub = bytearray(), bytearray()
    pred = int(P[bq, bs])
    while True:
        if pred == 1:
            bq -= 1; bs -= 1
            aq.append(q[bq]); asub.append(s[bs])
        elif pred == 2:
            bq -= 1
            aq.append(q[bq]); asub.append(0x5F)
        elif pred == 3:
            bs -= 1
            aq.append(0x5F); asub.append(s[bs])
        else:
            aq.append(0x5F); asub.append(0x5F)
        pred = int(P[bq, bs])
        if pred == 0:
            break
    return bv, bytes(aq[::-1]), bytes(asub[::-1])


def _size_t(x):
    return x & 0xFFFFFFFFFFFFFFFF


def make_semi_global_alignment(seq1, seq2, subject):
    """(score, aligned query, aligned subject, reverse): mate 1's alignment in the orientation the reference picks.  The two sums
    are std::size_t there: a negative sum is a huge number.  Forward wins only if strictly greater."""
    fwd = align_semi_global(seq1, subject)
    rev = align_semi_global(reverse_complement(seq1), subject)
    score, scorer = _size_t(fwd[0]), _size_t(rev[0])
    if seq2:
        score = _size_t(score + align_semi_global(seq2, subject, backtrace=False)[0])
        scorer = _size_t(scorer + align_semi_global(reverse_complement(seq2), subject, backtrace=False)[0])
    return (fwd + (0,)) if score > scorer else (rev + (1,))
