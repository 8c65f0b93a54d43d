"""mcq_reduce alone (rows 8-11: sort, de-duplicate, window sweep, top list, rank fold) on the caller-made lists of
tests/reduce_lists.py, through Workspace.reduce_device, exact against the oracle's reduce of the same list (which
tests/test_reduce_lists.py holds to a plain reference on the same corpus): ncand and all four words of every candidate
below it.  The outputs are sized exactly, prefilled, and followed by guard words that must come back untouched.  Every
test computes the class of each of its lists -- the kernel and the branch of it the list meets, from its length, its
distinct keys, the word width and the flags, by the rules of mcq_reduce restated in reduce_lists.route -- and asserts
that every class it claims to cover is there.

CONFIGS is not the product of location forms x (P, M) x flags.  What decides the code that runs is the word width (the
u32 or the u64 kernels), the location form (how a word is decoded), the path flags, and the form the P top lists take
(reduce_lists.list_form): 'p1', 'lin' (every P > 1 without MCQ_FOLD_BY_LISTS, and without MCQ_QUIRK_SEQ_DROP on a table
with sequence-level taxa), 'lanes' (P lists in a wave's lanes: pow2ceil(P) x M <= 64) and 'big' (P lists in the workgroup
kernel's LDS, BIG = 1, which then takes every list).  The pairs are chosen so that every kernel -- first wave stage u32
(de-duplicating with both sweeps, raw sort) and u64, second wave stage, workgroup kernel u32 and u64 in its LDS and its
global-scratch form -- meets every list form it can meet, every location form meets every list form, each of the eight
(P, M) pairs and each flag occurs, and MCQ_QUIRK_SEQ_DROP runs on the world with sequence-level taxa (where it changes
the list form) and on the one without (where it must not).  test_configs_cover_every_kernel_and_list_form checks that."""
import functools
import importlib

import numpy as np
import pytest
import torch

import reduce_lists as rl
from oracle import mc_oracle as orc

pytestmark = pytest.mark.gpu

GUARD = 0xA5A5A5A5
PAD = 64
FORMS = ("fields32", "gw", "loc64")
PM = [(1, 1), (1, 16), (2, 2), (3, 4), (8, 8), (32, 4), (64, 1), (64, 16)]
FLAG = {"0": 0, "raw": rl.FORCE_RAW_SORT, "no16": rl.NO_WAVE16, "block": rl.FORCE_BLOCK_PATH, "lists": rl.FOLD_BY_LISTS,
        "seqdrop": rl.QUIRK_SEQ_DROP}
# (location form, P, M, flag names, world with sequence-level taxa, insert_size_max)
CONFIGS = [
    # P = 1
    ("fields32", 1, 1, ("0",), False, 0),
    ("fields32", 1, 16, ("raw",), False, 0),
    ("gw", 1, 16, ("block",), False, 0),                    # BIG = 0 at P = 1 for every list
    ("gw", 1, 1, ("no16",), False, 0),
    ("loc64", 1, 1, ("0",), False, 0),
    ("loc64", 1, 16, ("0",), False, rl.INSERT_HUGE),        # the m >= 2^31 branch of range_width
    # rows 10-11 as one selection
    ("gw", 2, 2, ("0",), False, 0),
    ("gw", 3, 4, ("no16",), False, 0),                      # P no power of two: the fold keeps ranks 0 and 1 only
    ("loc64", 8, 8, ("0",), False, 0),
    ("fields32", 32, 4, ("0",), False, 0),                  # was 'big' once; make_opt now turns it into 'lin', BIG = 0
    ("loc64", 64, 1, ("block",), False, 0),
    ("fields32", 64, 16, ("0",), False, rl.INSERT_HUGE),
    ("fields32", 8, 8, ("seqdrop",), False, 0),             # no sequence-level taxa: still one selection
    ("fields32", 3, 4, ("raw",), False, 0),
    # P lists in a wave's lanes
    ("fields32", 2, 2, ("lists",), False, 0),
    ("loc64", 8, 8, ("lists",), False, 0),                  # 8 x 8 = 64 lanes: the last shape that fits
    ("gw", 3, 4, ("lists",), False, 0),
    ("gw", 64, 1, ("lists", "raw"), False, 0),
    ("fields32", 2, 2, ("seqdrop",), True, 0),
    ("loc64", 8, 8, ("seqdrop", "raw"), True, 0),
    ("gw", 2, 2, ("seqdrop", "block"), True, 0),
    ("fields32", 3, 4, ("lists", "no16"), True, 0),
    # P lists in the workgroup kernel's LDS
    ("fields32", 32, 4, ("lists",), False, 0),
    ("loc64", 64, 16, ("lists",), False, 0),
    ("gw", 32, 4, ("seqdrop",), True, 0),
    ("gw", 64, 16, ("lists", "seqdrop"), True, 0),
]
CFG_IDS = ["%s-P%d-M%d-%s%s%s" % (f, P, M, "+".join(fl), "-seqtaxa" if sq else "", "-ins2^33" if ins else "") for f, P, M, fl, sq, ins in CONFIGS]

LIST_FORMS = ["p1"] * 6 + ["lin"] * 8 + ["lanes"] * 8 + ["big"] * 4         # of CONFIGS, in its order
U32_WAVE = {"wave-dedup-regs", "wave-dedup-weighted", "wave-raw"}
BLOCK = {"block-lds", "block-global"}


def _flags(names):
    f = 0
    for n in names:
        f |= FLAG[n]
    return f


def _expected_classes(loc_bytes, flags, form, insert):
    """the classes a batch of the whole corpus must show under one configuration"""
    if (flags & rl.FORCE_BLOCK_PATH) or form == "big":
        return BLOCK | {"block-empty"}
    if loc_bytes == 8:
        return BLOCK | {"wave-empty", "wave64"}
    want = BLOCK | {"wave-empty", "wave-raw"} | (set() if flags & rl.NO_WAVE16 else {"wave16"})
    if not (flags & rl.FORCE_RAW_SORT):
        want |= {"wave-dedup-weighted"} | (set() if insert else {"wave-dedup-regs"})
    return want


@pytest.fixture(scope="module")
def eng():
    return importlib.import_module("metacache-mpi_amd.engine")


def _dev():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _world(seq_level):
    """the world, its oracle and its corpus, interleaved: (world, oracle, lists, query_len, what, T, D)"""
    w = rl.World(seq_level)
    odb = orc.OracleDb(w.keys, w.off, w.locs, w.tgt2tax, winstride=rl.TGT_STRIDE)
    lists, qlen, what = rl.flatten(rl.corpus(w))
    order = np.random.default_rng(3).permutation(len(lists))            # every length class next to every other
    lists, qlen, what = [lists[i] for i in order], qlen[order], [what[i] for i in order]
    T = np.array([len(x) for x in lists])
    D = np.array([len(np.unique(x)) for x in lists])
    return w, odb, lists, qlen, what, T, D


@functools.lru_cache(maxsize=None)
def _handle(seq_level, form, lmax=rl.LMAX, max_queries=2048):
    eng = importlib.import_module("metacache-mpi_amd.engine")
    w = _world(seq_level)[0]
    dbflags = {"fields32": 0, "gw": eng.MCQ_DB_LOCS_GW, "loc64": eng.MCQ_DB_LOCS_64}[form]
    db = eng.Database(w.keys, w.off, w.locs, w.tgt2tax, winstride=rl.TGT_STRIDE, flags=dbflags)
    assert db.loc_bytes() == (8 if form == "loc64" else 4)
    assert (db.layout()["loc_format"] == eng.MCQ_LOC_GLOBAL_WINDOW) == (form == "gw")
    if form == "fields32":              # the largest window id the bit field can hold is in use
        assert db.win_bits() == int(rl.W_MAX - 1).bit_length()
    ws = eng.Workspace(db, max_queries, 1, max_locs_per_query=lmax)
    return db, ws


def _reduce(eng, seq_level, form, lists, qlen, P, M, flags, insert=0, lmax=rl.LMAX, handle=None):
    """one mcq_reduce call on these lists, checked: guards, every served query against the oracle, the refused ones,
    MCQ_E_CAPACITY exactly when there are any, the statistics.  Returns the class of every list."""
    w, odb = _world(seq_level)[:2]
    db, ws = handle or _handle(seq_level, form)
    nq = len(lists)
    lform = rl.list_form(P, M, flags, seq_level)
    T = [len(x) for x in lists]
    cls = [rl.route(T[q], len(np.unique(lists[q])) if T[q] <= rl.LCAP_WAVE else -1, rl.num_windows_of(qlen[q], insert), db.loc_bytes(),
                    flags, lform, lmax) for q in range(nq)]
    loc_off = np.zeros(nq + 1, np.int64)
    loc_off[1:] = np.cumsum(T)
    allv = rl.to_native(np.concatenate(lists + [np.zeros(0, np.uint64)]), db)
    dev = _dev()
    dl = torch.from_numpy(allv.view(np.int32 if db.loc_bytes() == 4 else np.int64).copy()).to(dev) if allv.size else \
        torch.zeros(1, dtype=torch.int64, device=dev)
    doff = torch.from_numpy(loc_off).to(dev)
    dq = torch.from_numpy(np.ascontiguousarray(qlen, np.uint32).view(np.int32).copy()).to(dev)
    # exactly nq x M x 4 and nq words, then the guard; the outputs themselves start as the guard too: every word that
    # must be written shows when it was not
    cands = torch.full((nq * M * 4 + PAD,), GUARD - (1 << 32), dtype=torch.int32, device=dev)
    ncand = torch.full((nq + PAD,), GUARD - (1 << 32), dtype=torch.int32, device=dev)
    ws.reduce_device(nq, doff.data_ptr(), dl.data_ptr(), dq.data_ptr(), cands.data_ptr(), ncand.data_ptr(), max_cand=M, emulate_ranks=P,
                     insert_size_max=insert, flags=flags, stream=torch.cuda.current_stream(dev).cuda_stream)
    n_refused = cls.count("capacity")
    stats = None
    if n_refused:
        with pytest.raises(eng.McqError) as e:
            ws.sync()
        assert e.value.code == eng.MCQ_E_CAPACITY and ("%d queries exceeded" % n_refused) in str(e.value), str(e.value)
    else:
        stats = ws.sync()
    gc = cands.cpu().numpy().view(np.uint32)
    gn = ncand.cpu().numpy().view(np.uint32)
    assert (gc[nq * M * 4:] == GUARD).all() and (gn[nq:] == GUARD).all(), "written behind the outputs"
    gc = gc[:nq * M * 4].reshape(nq, M, 4)
    quirk = 1 if flags & rl.QUIRK_SEQ_DROP else 0
    for q, lst in enumerate(lists):
        ctx = "query %d (%s, %d words) %s P=%d M=%d flags=%s insert_size_max=%d query_len=%d: " % (
            q, cls[q], T[q], form, P, M, hex(flags), insert, int(qlen[q]))
        if cls[q] == "capacity":
            assert gn[q] == 0, ctx
            continue
        oc, on = odb.reduce_query(lst, int(qlen[q]), max_cand=M, emulate_ranks=P, insert_size_max=insert, quirk_seq_drop=quirk)
        assert gn[q] == on, ctx + "ncand %d, oracle %d" % (int(gn[q]), on)
        assert np.array_equal(gc[q, :on], oc[:on]), ctx + "%s, oracle %s" % (gc[q, :on].tolist(), oc[:on].tolist())
    if stats is not None:
        assert stats["n_queries"] == nq
        assert stats["n_locations"] == sum(T), (stats["n_locations"], sum(T))
    return cls


# ====================================================================================== the whole corpus, interleaved
def test_configs_cover_every_kernel_and_list_form():
    """what the choice of CONFIGS promises (see the head of this file), computed from the corpus and the routing rules"""
    T, D = _world(False)[5:7]
    qlen = _world(False)[3]
    met = set()                 # (class, list form, location form)
    for form, P, M, names, seq, ins in CONFIGS:
        flags, b = _flags(names), 8 if form == "loc64" else 4
        lf = rl.list_form(P, M, flags, seq)
        for t, d, q in zip(T, D, qlen):
            met.add((rl.route(int(t), int(d), rl.num_windows_of(q, ins), b, flags, lf), lf, form))
    assert [rl.list_form(P, M, _flags(names), seq) for _, P, M, names, seq, _ in CONFIGS] == LIST_FORMS
    assert {(P, M) for _, P, M, _, _, _ in CONFIGS} == set(PM)
    assert {n for c in CONFIGS for n in c[3]} == set(FLAG)
    assert any(c[4] and "seqdrop" in c[3] for c in CONFIGS) and any(not c[4] and "seqdrop" in c[3] for c in CONFIGS)
    assert {(lf, f) for _, lf, f in met} == {(lf, f) for lf in ("p1", "lin", "lanes", "big") for f in FORMS}
    for lf in ("p1", "lin", "lanes"):
        u32 = {c for c, l, f in met if l == lf and f != "loc64"}
        assert u32 >= U32_WAVE | BLOCK | {"wave16"}, (lf, u32)
        assert {c for c, l, f in met if l == lf and f == "loc64"} >= BLOCK | {"wave64"}, lf
        for f in ("fields32", "gw"):    # the two 32-bit words are decoded differently in every kernel
            assert {c for c, l, ff in met if l == lf and ff == f} & U32_WAVE and ("block-lds", lf, f) in met, (lf, f)
    for f in FORMS:
        assert {c for c, l, ff in met if l == "big" and ff == f} == BLOCK | {"block-empty"}, f
    # the three candidate-list forms of the workgroup kernel: BIG = 0 under lin, BIG = 0 at P = 1, BIG = 1
    for lf in ("lin", "p1", "big"):
        assert {c for c, l, _ in met if l == lf} >= BLOCK


@pytest.mark.parametrize("cfg", CONFIGS, ids=CFG_IDS)
def test_whole_corpus_interleaved(eng, cfg):
    """one batch of every list of the corpus, the length classes interleaved"""
    form, P, M, names, seq, ins = cfg
    flags = _flags(names)
    _, _, lists, qlen, what, T, D = _world(seq)
    cls = _reduce(eng, seq, form, lists, qlen, P, M, flags, insert=ins)
    lf = rl.list_form(P, M, flags, seq)
    assert lf == LIST_FORMS[CONFIGS.index(cfg)]
    assert set(cls) == _expected_classes(8 if form == "loc64" else 4, flags, lf, ins), (lf, set(cls))
    # interleaved: every class has a neighbour of another class
    assert all(any(cls[i] == c and cls[i + 1] != c for i in range(len(cls) - 1)) for c in set(cls))
    # both sides of every routing edge, and the exact capacity
    assert set(rl.EDGE_T) <= set(T.tolist()) and int(T.max()) == rl.LMAX


# ====================================================================================== batch shapes
def _pick(cls, want, n, rng, T, longest=None):
    """indices of n lists whose class is in `want` (shorter than `longest`), in a random order"""
    idx = [i for i, c in enumerate(cls) if c in want and (longest is None or T[i] <= longest)]
    assert len(idx) >= n, (want, len(idx), n)
    return [int(i) for i in rng.choice(idx, size=n, replace=False)]


@pytest.mark.parametrize("form,P,M", [("fields32", 1, 4), ("gw", 2, 2), ("loc64", 3, 4)])
def test_batch_shapes(eng, form, P, M):
    """batches of one length class only (nothing for the first stage, an empty middle queue, an empty workgroup queue, no
    queue at all), a single query of every class, and 1, 7, 8 and 9 queued queries: the queues hand out slots in chunks
    of MCQ_OVF_CHUNK = 8 and fill the rest of a chunk with empty markers"""
    _, _, lists, qlen, what, T, D = _world(False)
    b = 8 if form == "loc64" else 4
    lf = rl.list_form(P, M, 0, False)
    cls = [rl.route(int(t), int(d), rl.num_windows_of(q), b, 0, lf) for t, d, q in zip(T, D, qlen)]
    rng = np.random.default_rng(11)
    wave = {"wave64"} if b == 8 else U32_WAVE
    mid = {"wave16"} if b == 4 else set()
    run = lambda idx: _reduce(eng, False, form, [lists[i] for i in idx], qlen[idx], P, M, 0)
    queues = lambda got: {rl.queue_of(c) for c in got}

    got = run(_pick(cls, wave | {"wave-empty"}, 60, rng, T))
    assert queues(got) == {"none"}                                      # both queues empty
    got = run(_pick(cls, mid | BLOCK, 24, rng, T, 8200))
    assert queues(got) == ({"mid", "block"} if b == 4 else {"block"})   # nothing for the first stage
    got = run(_pick(cls, wave, 40, rng, T) + _pick(cls, BLOCK, 10, rng, T, 8200))
    assert queues(got) == {"none", "block"}                             # an empty middle queue
    if b == 4:
        got = run(_pick(cls, wave, 40, rng, T) + _pick(cls, mid, 10, rng, T))
        assert queues(got) == {"none", "mid"}                           # an empty workgroup queue
        got = run(_pick(cls, mid, 12, rng, T))
        assert queues(got) == {"mid"}
    singles = set()
    for c in sorted(set(cls)):                                          # nq = 1
        got = run(_pick(cls, {c}, 1, rng, T))
        singles |= set(got)
    assert singles == _expected_classes(b, 0, lf, 0)
    assert rl.OVF_CHUNK == 8
    for k in (1, 7, 8, 9):
        for alone in (True, False):
            idx = _pick(cls, BLOCK, k, rng, T, 2000) + (_pick(cls, mid, k, rng, T) if mid else [])
            if not alone:
                idx += _pick(cls, wave | {"wave-empty"}, 20, rng, T)
            idx = [idx[i] for i in rng.permutation(len(idx))]
            got = run(idx)
            assert sum(c in BLOCK for c in got) == k and sum(c in mid for c in got) == (k if mid else 0)
            assert (len(got) == k * (2 if mid else 1)) == alone


# ====================================================================================== capacity
@pytest.mark.parametrize("form,P,M,names", [("fields32", 1, 2, ("0",)), ("loc64", 2, 2, ("0",)), ("gw", 32, 4, ("lists",)),
                                            ("fields32", 8, 8, ("lists", "block"))], ids=["fields32-p1", "loc64-lin", "gw-big", "fields32-lanes-block"])
def test_capacity_refusal(eng, form, P, M, names):
    """one query of lmax + 1 words among others: it gets ncand = 0, the sync reports MCQ_E_CAPACITY for exactly one query,
    every other query of the batch -- one of exactly lmax words among them -- is still exact, and the next batch on the
    same workspace is clean"""
    w, _, lists, qlen, what, T, D = _world(False)
    flags = _flags(names)
    b = 8 if form == "loc64" else 4
    lf = rl.list_form(P, M, flags, False)
    cls = [rl.route(int(t), int(d), rl.num_windows_of(q), b, flags, lf) for t, d, q in zip(T, D, qlen)]
    rng = np.random.default_rng(12)
    idx = []
    for c in sorted(set(cls)):
        idx += _pick(cls, {c}, 3, rng, T, 9000)
    idx.append(int(np.nonzero(T == rl.LMAX)[0][0]))
    idx = [idx[i] for i in rng.permutation(len(idx))]
    t = w.targets_with(rl.W_MAX)[0]
    over = rng.permutation(np.concatenate([rl.loc(t, np.arange(rl.LMAX - 100)), np.full(101, rl.loc(3, 60))]))
    assert len(over) == rl.LMAX + 1
    at = len(idx) // 2
    batch = [lists[i] for i in idx[:at]] + [over] + [lists[i] for i in idx[at:]]
    ql = np.concatenate([qlen[idx[:at]], np.array([150], np.uint32), qlen[idx[at:]]])
    got = _reduce(eng, False, form, batch, ql, P, M, flags)
    assert got.count("capacity") == 1 and got[at] == "capacity"
    assert set(got) == set(cls) | {"capacity"} and rl.LMAX in [len(x) for x, c in zip(batch, got) if c == "block-global"]
    again = _reduce(eng, False, form, [lists[i] for i in idx], qlen[idx], P, M, flags)
    assert "capacity" not in again


# ====================================================================================== counts beyond 16 bits
@pytest.mark.parametrize("form,P,M", [("fields32", 1, 2), ("loc64", 2, 2)])
def test_66000_copies_of_one_location(eng, form, P, M):
    """(i) the count of one (target, window) must not wrap a 16-bit counter anywhere in the workgroup kernel's
    global-scratch form; a workspace of its own with lmax = 2^17"""
    w, odb = _world(False)[:2]
    lmax = 1 << 17
    lists = rl.counter_wrap_lists(w)
    lists = [lists[0], np.full(5, rl.loc(1, 1)), lists[1], lists[2]]
    db, ws = _handle.__wrapped__(False, form, lmax=lmax, max_queries=8)
    try:
        qlen = np.full(len(lists), 150, np.uint32)
        got = _reduce(eng, False, form, lists, qlen, P, M, 0, lmax=lmax, handle=(db, ws))
        assert got.count("block-global") == 3 and max(len(x) for x in lists) > rl.LMAX
        oc, on = odb.reduce_query(lists[0], 150, max_cand=M, emulate_ranks=P)
        assert on == 1 and oc[0, 1] == 66000 > 0xFFFF
        oc, on = odb.reduce_query(lists[2], 150, max_cand=M, emulate_ranks=P)
        assert on == 2 and oc[0, 1] == 66000 and oc[1, 1] == 30000
    finally:
        ws.close()
        db.close()
