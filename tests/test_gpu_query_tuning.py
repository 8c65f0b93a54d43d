"""The bucket rules inside the streaming loader (mcq_parts_builder_set_bucket_limit) and a tuned query sketcher on the handle:
the shard files streamed through PartsBuilder with a rule, the fixture's reads queried, candidate for candidate against
oracle.mc_oracle on the union of the NumPy-filtered per-rank tables (tests/bucket_limit_ref.py on oracle/dbfile.py's parse);
a handle with query windows 64 / 64 and sketch 8 against the oracle given the same query sketcher; and a builder without
the call against one with both rules off and against the unfiltered union."""
import functools
import importlib

import numpy as np
import pytest

import bucket_limit_ref as ref
from golden_util import Fixture
from oracle import dbfile
from oracle import mc_oracle as orc

pytestmark = pytest.mark.gpu


def _mods():
    importlib.import_module("metacache-mpi_amd").build_host()
    return importlib.import_module("metacache-mpi_amd.engine"), importlib.import_module("metacache-mpi_amd.host")


@functools.lru_cache(maxsize=None)
def _fixture(tag, P):
    fx = Fixture(tag, P)
    return fx, orc.pack_reads(fx.interleaved())


def _streamed_db(fx, P, rule=None, chunk=1000, sketch=None):
    """the handle of the whole table by the streaming route; rule = (keep_first, remove_above) or None = no call;
    sketch = (sketch_size, winlen, winstride) of the queries or None = the database's.  -> (db, (shrunk, removed), t2t)"""
    eng, host = _mods()
    rdb = host.RefDb(fx.shard_paths[0][: -len(".db_0")], P, meta_only=True)
    i = rdb.info
    s, wl, ws = sketch or (i.q_sketch_size, i.q_winlen, i.q_winstride)
    pb = eng.PartsBuilder(rdb.tgt_windows(), k=i.k, sketch_size=s, winlen=wl, winstride=ws, tgt_winstride=i.winstride, expected_locations=i.n_locs)
    if rule is not None:
        pb.set_bucket_limit(*rule)
    for r in range(P):
        for f, t, w in rdb.stream(r, chunk):              # (whole key records of one file per chunk)
            pb.add(f, t, w)
    counts = pb.bucket_counts()
    parts = pb.finish()
    t2t = rdb.tgt2tax(fx.lowest)
    db = parts.database(t2t.ctypes.data, n_shards=1, shard_id=0, device_ptrs=False)
    parts.close()
    return db, counts, t2t


def _query(eng, db, fx, packed, P):
    bases, seq_off = packed
    ws = eng.Workspace(db, len(fx.names), len(bases))
    cands, ncand = ws.query_host(bases, seq_off, True, max_cand=fx.maxcand, emulate_ranks=P, flags=eng.MCQ_QUIRK_SEQ_DROP)
    ws.close()
    return cands, ncand


def _oracle(fx, shards, t2t, packed, P, sketch=None):
    p = fx.params
    s, wl, ws = sketch or (p["qs"], p["qwinlen"], p["qwinstride"])
    rk, ro, rl = dbfile.union_shards(shards)
    odb = orc.OracleDb(rk, ro, rl, t2t, k=p["qk"], s=s, winlen=wl, winstride=ws, tgt_winstride=p["winstride"])
    return odb.query(packed[0], packed[1], True, max_cand=fx.maxcand, emulate_ranks=P, quirk_seq_drop=1)


def _same(cands, ncand, oc, on):
    assert np.array_equal(ncand, on)
    for q in range(len(on)):
        assert np.array_equal(cands[q, :on[q]], oc[q, :on[q]]), q


@pytest.mark.parametrize("P", [2, 4])
@pytest.mark.parametrize("rule", [(40, 0), (0, 39), (16, 60)], ids=["shrink40", "remove39", "remove60_shrink16"])
def test_overpop_through_the_builder_with_a_rule(P, rule):
    eng, _ = _mods()
    fx, packed = _fixture("overpop", P)
    db, (shrunk, removed), t2t = _streamed_db(fx, P, rule)
    want = [ref.bucket_limit(np.repeat(s["keys"], np.diff(s["off"]).astype(np.int64)), s["tgt"], s["win"], *rule) for s in fx.shards]
    assert (shrunk, removed) == (sum(w[3] for w in want), sum(w[4] for w in want))
    assert shrunk + removed > 0                             # (the long buckets, up to 100, are there)
    filtered = [ref.filter_shard(s, *rule) for s in fx.shards]
    _same(*_query(eng, db, fx, packed, P), *_oracle(fx, filtered, t2t, packed, P))
    # ... and the rule changes what the reads find: the oracle on the unfiltered tables answers otherwise
    oc, on = _oracle(fx, fx.shards, t2t, packed, P)
    cands, ncand = _query(eng, db, fx, packed, P)
    assert not (np.array_equal(ncand, on) and all(np.array_equal(cands[q, :on[q]], oc[q, :on[q]]) for q in range(len(on))))
    db.close()


def test_tuned_query_sketcher_on_the_handle():
    eng, _ = _mods()
    fx, packed = _fixture("mini", 4)
    sketch = (8, 64, 64)
    db, counts, t2t = _streamed_db(fx, 4, None, sketch=sketch)
    assert counts == (0, 0)
    _same(*_query(eng, db, fx, packed, 4), *_oracle(fx, fx.shards, t2t, packed, 4, sketch))
    db.close()


@pytest.mark.parametrize("tag,P", [("overpop", 2), ("mini", 4)])
def test_builder_without_the_call_is_unchanged(tag, P):
    eng, _ = _mods()
    fx, packed = _fixture(tag, P)
    plain, c0, t2t = _streamed_db(fx, P, None)
    off, c1, _ = _streamed_db(fx, P, (0, 0))
    assert c0 == (0, 0) and c1 == (0, 0)
    a, b = plain.layout(), off.layout()
    a.pop("gw_offsets"), b.pop("gw_offsets")               # (a device address)
    assert a == b
    a, b = _query(eng, plain, fx, packed, P), _query(eng, off, fx, packed, P)
    _same(*a, *b)
    _same(*a, *_oracle(fx, fx.shards, t2t, packed, P))
    plain.close(); off.close()
