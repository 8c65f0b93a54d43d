"""Interleaved read texts for the tests of MCQ_READS_INTERLEAVED and -pairseq: the pairs of the `mini` fixture, record
2q the first mate and record 2q+1 the second, as FASTQ or as FASTA wrapped at 60 columns."""
from golden_util import Fixture


def interleaved_records(odd=False, tag="mini", P=4):
    """[(header, sequence)] as bytes: the fixture's pairs (they hold 15 bp and 2 kb reads) with an N read and a lowercase
    read put in; odd: one more record, which has no mate"""
    fx = Fixture(tag, P)
    recs = []
    for q, (name, a, b) in enumerate(zip(fx.names, fx.r1, fx.r2)):
        if q == 3:
            a = a[:20] + "N" * 7 + a[27:]
        if q == 5:
            b = b.lower()
        recs += [((name + " first mate").encode(), a.encode()), ((name + "/2").encode(), b.encode())]
    if odd:
        recs.append((b"lonely read", fx.r1[0][::-1].encode()))
    return recs


def deinterleave(recs):
    return recs[0::2], recs[1::2]


def render(recs, fmt, final_newline=True, eol=b"\n"):
    out = []
    for h, s in recs:
        if fmt == "fastq":
            out += [b"@" + h, s, b"+", b"I" * len(s)]
        else:
            out += [b">" + h] + [s[k:k + 60] for k in range(0, len(s), 60)]
    text = eol.join(out) + eol
    return text if final_newline else text[:-len(eol)]
