"""mcq_align (include/mcq.h, csrc/mcq_align.hip) through Workspace.align: the reference's make_semi_global_alignment of every query
against its subject, bit for bit.  Expected values: the recorded cases of tests/golden/align/cases.json.gz (what the reference's
align_semi_global returned, both orientations of every query), and tests/align_ref.py -- which tests/test_align_ref.py holds to
the same cases -- for mate 2's score-only passes and for the one pair at the kernel's capacities.

The shapes are those of the fixture (tests/golden/make_golden_alignment.py): query lengths around the strip width 8 and around a
wave's 64 rows in flight, subject lengths around one and two waves of columns and around one panel of 512 columns, 4096 against 65,
empty sequences, homopolymers, overhangs, lower case and N, the scores of -1, and pairs whose predecessor matrix exceeds the 10240
LDS words (65 x 4096, 100 x 900, 300 x 600, 150 x 1100) next to those that fit."""
import importlib

import numpy as np
import pytest
import torch  # noqa: F401  (first: the library then binds to the HIP runtime torch brings along)

import align_ref
from test_align_ref import load_cases

pytestmark = pytest.mark.gpu

FILL = 0x2E
LDS_WORDS = 10240           # AL_LDS_WORDS of csrc/mcq_align.hip: predecessor words (8 cells each) a wave keeps in LDS


def _eng():
    return importlib.import_module("metacache-mpi_amd.engine")


_world = {}


def world():
    """one tiny table (mcq_align reads none), one workspace, the recorded cases by (query, subject)"""
    if not _world:
        eng = _eng()
        db = eng.Database(np.array([5], np.uint32), np.array([0, 1], np.uint64), np.array([0], np.uint64), np.array([1], np.uint32))
        _world["db"] = db
        _world["ws"] = eng.Workspace(db, 1024, 1 << 20)
        cases = load_cases()
        _world["cases"] = cases
        _world["rec"] = {(q, s): (sc, aq, asub) for q, s, sc, aq, asub in cases}
    return _world


def size_t(x):
    return x & 0xFFFFFFFFFFFFFFFF


def expected(rec, m1, m2, sub):
    """(score, aligned query, aligned subject, reverse) from the recorded alignments of mate 1; mate 2 adds the restatement's scores"""
    f, r = rec[(m1, sub)], rec[(align_ref.reverse_complement(m1), sub)]
    sf, sr = size_t(f[0]), size_t(r[0])
    if m2:
        sf = size_t(sf + align_ref.align_semi_global(m2, sub, backtrace=False)[0])
        sr = size_t(sr + align_ref.align_semi_global(align_ref.reverse_complement(m2), sub, backtrace=False)[0])
    return (f + (0,)) if sf > sr else (r + (1,))


def pack(queries, subjects, paired, ranges, on=None):
    """the leading arguments of Workspace.align: bases, seq_off, paired, subjects buffer, jobs.  ranges: the sequences lie in the buffer in reverse order with a gap in between"""
    seqs = [m for q in queries for m in (q if paired else q[:1])]
    if ranges:
        buf, pos, off = bytearray(b"#" * 3), {}, []
        for i in reversed(range(len(seqs))):
            pos[i] = len(buf); buf += seqs[i] + b"#"
        for i in range(len(seqs)):
            off += [pos[i], pos[i] + len(seqs[i])]
        bases, seq_off = bytes(buf), np.array(off, np.uint64)
    else:
        bases = b"".join(seqs)
        seq_off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    sub_buf, jobs = bytearray(b"xx"), []
    for i, s in enumerate(subjects):
        jobs.append((len(sub_buf), len(s), 1 if on is None or on[i] else 0))
        sub_buf += s + b"x"
    return bases, seq_off, paired, bytes(sub_buf), jobs


def check(got, exp, ctx):
    for q, e in enumerate(exp):
        if e is None:
            continue
        assert got["status"][q] == 0, (ctx, q, got["status"][q])
        assert (int(got["score"][q]), got["query"][q], got["subject"][q], int(got["reverse"][q])) == e, \
            (ctx, q, int(got["score"][q]), int(got["reverse"][q]), e[0], e[3], got["query"][q][:60], e[1][:60])
        L = len(e[1])
        assert got["length"][q] == L
        assert (got["text_query"][q, L:] == FILL).all() and (got["text_subject"][q, L:] == FILL).all(), (ctx, q)


@pytest.mark.parametrize("ranges", [False, True], ids=["offsets", "ranges"])
def test_single_end_every_recorded_case(ranges):
    w = world()
    cases = w["cases"]
    queries = [(c[0],) for c in cases]
    subjects = [c[1] for c in cases]
    exp = [expected(w["rec"], c[0], b"", c[1]) for c in cases]
    assert {e[3] for e in exp} == {0, 1} and min(e[0] for e in exp) == -1
    words = [len(c[0]) * ((len(c[1]) + 7) // 8) for c in cases]
    assert min(w_ for w_ in words if w_) <= LDS_WORDS < max(words)          # both homes of the predecessors
    got = w["ws"].align(*pack(queries, subjects, False, ranges), ranges=ranges, fill=FILL)
    check(got, exp, "single")


@pytest.mark.parametrize("ranges", [False, True], ids=["offsets", "ranges"])
def test_paired_cases(ranges):
    """mate 2 only moves the choice of orientation: its own alignment is never printed"""
    w = world()
    small = [c for c in w["cases"] if len(c[1]) <= 129] + [c for c in w["cases"] if len(c[1]) in (467, 900)][:6]
    queries, subjects = [], []
    for k, c in enumerate(small):
        m2 = (align_ref.reverse_complement(c[0]), small[(k + 1) % len(small)][0], b"", c[0])[k % 4]
        queries.append((c[0], m2)); subjects.append(c[1])
    queries += [(b"AC", b"T"), (b"C", b""), (b"", b"ACGT")]             # forward sum negative, reverse sum positive; empty mates
    subjects += [b"G", b"G", b"ACGTACGT"]
    rec = dict(w["rec"])
    for q, s in ((b"AC", b"G"), (b"GT", b"G"), (b"C", b"G"), (b"G", b"G"), (b"", b"ACGTACGT")):
        rec[(q, s)] = align_ref.align_semi_global(q, s)
    exp = [expected(rec, q[0], q[1], s) for q, s in zip(queries, subjects)]
    assert exp[-3][3] == 0 and exp[-3][0] == -1 and exp[-2] == (-1, b"C", b"G", 0) and exp[-1] == (0, b"_", b"_", 1)
    got = w["ws"].align(*pack(queries, subjects, True, ranges), ranges=ranges, fill=FILL)
    check(got, exp, "paired")


def test_queries_switched_off_are_left_alone():
    w = world()
    cases = w["cases"][:48]
    on = [k % 3 != 0 for k in range(len(cases))]
    exp = [expected(w["rec"], c[0], b"", c[1]) if o else None for c, o in zip(cases, on)]
    got = w["ws"].align(*pack([(c[0],) for c in cases], [c[1] for c in cases], False, False, on=on), fill=FILL)
    check(got, exp, "on/off")
    for q, o in enumerate(on):
        if not o:
            assert (got["length"][q], got["status"][q]) == (0, 0)
            assert (got["text_query"][q] == FILL).all() and (got["text_subject"][q] == FILL).all()


def test_a_query_beyond_a_capacity_is_reported_and_its_slots_stay_untouched():
    eng, w = _eng(), world()
    by_len = {}
    for c in w["cases"]:
        by_len.setdefault((len(c[0]), len(c[1])), c)
    ok, long_q, long_s = by_len[(65, 129)], by_len[(150, 467)], by_len[(64, 511)]
    # single-end: bounds 65 / 129; query 1 has a mate of 150 bases, query 3 a subject of 511
    picks = [ok, long_q, by_len[(64, 128)], long_s, by_len[(63, 127)]]
    got = w["ws"].align(*pack([(c[0],) for c in picks], [c[1] for c in picks], False, False), max_query=65, max_subject=129, text_cap=65 + 129, fill=FILL)
    exp = [expected(w["rec"], c[0], b"", c[1]) for c in picks]
    exp[1] = exp[3] = None
    check(got, exp, "capacity")
    assert got["status"].tolist() == [0, eng.MCQ_ALIGN_QUERY_LONG | eng.MCQ_ALIGN_SUBJECT_LONG, 0, eng.MCQ_ALIGN_SUBJECT_LONG, 0]
    for q in (1, 3):
        assert got["length"][q] == 0
        assert (got["text_query"][q] == FILL).all() and (got["text_subject"][q] == FILL).all()
    # paired: only the second mate is too long
    got = w["ws"].align(*pack([(ok[0], long_q[0]), (ok[0], ok[0])], [ok[1], ok[1]], True, False), max_query=65, max_subject=129, fill=FILL)
    assert got["status"].tolist() == [eng.MCQ_ALIGN_QUERY_LONG, 0] and got["length"][0] == 0
    assert (got["text_query"][0] == FILL).all() and (got["text_subject"][0] == FILL).all()
    check(got, [None, expected(w["rec"], ok[0], ok[0], ok[1])], "capacity, paired")


def test_traceback_in_lds_and_in_scratch():
    """Where a job's predecessors go is decided per job, by its own rows x strips; max_subject only decides whether the call has
    scratch at all.  So: a 150 x 467 job, which fits the LDS words, under bounds that make no scratch and under max_subject 4096,
    which makes it (the job still traces in LDS: same answer); then a 100 x 900 job, which does not fit, alone in its call: that one
    traces from scratch."""
    w = world()
    c = next(c for c in w["cases"] if (len(c[0]), len(c[1])) == (150, 467))
    e = expected(w["rec"], c[0], b"", c[1])
    assert 150 * ((467 + 7) // 8) <= LDS_WORDS < 150 * (4096 // 8)
    for max_subject in (467, 4096):
        got = w["ws"].align(*pack([(c[0],)], [c[1]], False, False), max_query=150, max_subject=max_subject, fill=FILL)
        check(got, [e], "max_subject %d" % max_subject)
    c = next(c for c in w["cases"] if (len(c[0]), len(c[1])) == (100, 900))
    assert 100 * ((900 + 7) // 8) > LDS_WORDS
    got = w["ws"].align(*pack([(c[0],)], [c[1]], False, False), max_query=100, max_subject=900, fill=FILL)
    check(got, [expected(w["rec"], c[0], b"", c[1])], "100 x 900")


def test_scratch_and_lds_jobs_share_a_grid_clamped_by_the_scratch():
    """bounds at the capacities leave the 256 MiB of scratch room for 128 areas, so a batch of 640 queries runs on 128 waves, each
    striding over five queries: jobs that trace from scratch (100 x 900, 300 x 600, 150 x 1100) and jobs that trace in LDS follow
    one another on the same wave and in the same area"""
    eng, w = _eng(), world()
    words = eng.MCQ_ALIGN_MAX_QUERY * (eng.MCQ_ALIGN_MAX_SUBJECT // 8)
    n_areas = (256 << 20) // 2 // words
    assert n_areas == 128
    big = [c for c in w["cases"] if (len(c[0]), len(c[1])) in ((100, 900), (300, 600), (150, 1100))]
    small = [c for c in w["cases"] if 0 < len(c[0]) * ((len(c[1]) + 7) // 8) <= LDS_WORDS and len(c[1]) >= 63]
    assert len(big) >= 3 and len(small) >= 20
    picks = [(big[q % len(big)] if q % 3 == 0 else small[(7 * q) % len(small)]) for q in range(5 * n_areas)]
    exp = [expected(w["rec"], c[0], b"", c[1]) for c in picks]
    got = w["ws"].align(*pack([(c[0],) for c in picks], [c[1] for c in picks], False, False), max_query=eng.MCQ_ALIGN_MAX_QUERY,
                        max_subject=eng.MCQ_ALIGN_MAX_SUBJECT, fill=FILL)
    check(got, exp, "clamped grid")


def test_a_pair_at_the_capacities():
    eng, w = _eng(), world()
    rng = np.random.default_rng(7)
    sub = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), eng.MCQ_ALIGN_MAX_SUBJECT))
    m1 = bytearray(sub[1500:1500 + eng.MCQ_ALIGN_MAX_QUERY])
    for i in range(0, len(m1), 37):
        m1[i] = ord("N")
    del m1[500:503]
    m1 = bytes(m1) + b"ACG"
    assert len(m1) == eng.MCQ_ALIGN_MAX_QUERY
    e = align_ref.make_semi_global_alignment(m1, b"", sub)
    got = w["ws"].align(*pack([(m1,)], [sub], False, False), fill=FILL)
    check(got, [e], "%d x %d" % (len(m1), len(sub)))


def test_packed_batches_and_bad_bounds_are_refused():
    eng, w = _eng(), world()
    args = pack([(b"ACGT",)], [b"ACGT"], False, False)
    with pytest.raises(eng.McqError) as ei:
        w["ws"].align(*args, packed=True)
    assert ei.value.code == eng.MCQ_E_UNSUPPORTED
    for kw in (dict(max_query=eng.MCQ_ALIGN_MAX_QUERY + 1, max_subject=8, text_cap=8192),
               dict(max_query=8, max_subject=eng.MCQ_ALIGN_MAX_SUBJECT + 1, text_cap=8192),
               dict(max_query=8, max_subject=8, text_cap=15)):
        with pytest.raises(eng.McqError) as ei:
            w["ws"].align(*args, **kw)
        assert ei.value.code == eng.MCQ_E_ARG
