"""Clade exclusion (mcq_ws_set_exclusion / mcq_ws_set_query_clades; the reference's -exclude RANK) on every route of mcq_query.

Exclusion is DEFINED as a filter on a query's match list (remove_hits_on_rank, src/classification.cpp:141-157): the expected
result here is OracleDb.reduce_query on OracleDb.matches with the excluded targets' locations removed in Python.  The kernels
retire the excluded targets' run heads instead; that the two are the same thing is what this file checks, not what it assumes.
The truths come from the rewritten headers (tests/golden/<tag>/eval_headers.json) through the host library, as do the targets'
clade keys."""
import ctypes as C
import importlib
import json
import os

import numpy as np
import pytest

from golden_util import GOLDEN, Fixture
from oracle import dbfile
from oracle import mc_oracle as orc

pytestmark = pytest.mark.gpu

SPECIES, GENUS = 4, 6
CASES = [("mini", 2), ("mini", 4), ("tie", 2), ("noanc", 2)]
_worlds = {}


def _world(tag, P):
    """one fixture: oracle table, reads, clade keys at species and genus, and the expected lists (computed once, never changed)"""
    if (tag, P) in _worlds:
        return _worlds[(tag, P)]
    eng = importlib.import_module("metacache-mpi_amd.engine")
    host = importlib.import_module("metacache-mpi_amd.host")
    fx = Fixture(tag, P)
    keys, off, locs = dbfile.union_shards(fx.shards)
    p = fx.params
    kw = dict(k=p["qk"], winlen=p["qwinlen"], winstride=p["qwinstride"], tgt_winstride=p["winstride"])
    t2t = fx.tgt2tax()
    odb = orc.OracleDb(keys, off, locs, t2t, s=p["qs"], **kw)
    rdb = host.RefDb(fx.shard_paths[0][: -len(".db_0")], P)
    with open(os.path.join(GOLDEN, tag, "eval_headers.json")) as f:
        headers = json.load(f)
    truth = [rdb.ground_truth(h) for h in headers]
    bases, seq_off = orc.pack_reads(fx.interleaved())
    w = dict(eng=eng, fx=fx, odb=odb, table=(keys, off, locs, t2t), kw=dict(sketch_size=p["qs"], **kw), bases=bases, seq_off=seq_off,
             truth=truth, headers=headers, nq=len(fx.names), dbs={}, expect={}, tgt={}, qkey={})
    for rank in (SPECIES, GENUS):
        w["tgt"][rank] = rdb.clade_keys(rank)
        w["qkey"][rank] = np.array([rdb.taxon_clade(t, rank) for t in truth], np.uint32)
    w["matches"] = [odb.matches(a, b) for a, b in zip(fx.r1, fx.r2)]
    _worlds[(tag, P)] = w
    return w


def _expected(w, rank, max_cand, ranks, qkey=None):
    """reduce_query on the match lists without the excluded targets' locations"""
    key = (rank, max_cand, ranks, None if qkey is None else qkey.tobytes())
    if key not in w["expect"]:
        fx, tgt = w["fx"], w["tgt"][rank]
        qk = w["qkey"][rank] if qkey is None else qkey
        cands = np.zeros((w["nq"], max_cand, 4), np.uint32)
        ncand = np.zeros(w["nq"], np.uint32)
        for q in range(w["nq"]):
            m = w["matches"][q]
            if qk[q] != w["eng"].MCQ_CLADE_KEEP_ALL:
                m = m[tgt[(m >> np.uint64(32)).astype(np.int64)] != qk[q]]
            c, n = w["odb"].reduce_query(m, len(fx.r1[q]) + len(fx.r2[q]), max_cand=max_cand, emulate_ranks=ranks)
            cands[q], ncand[q] = c, n
        w["expect"][key] = (cands, ncand)
    return w["expect"][key]


def _db(w, flags=0):
    if flags not in w["dbs"]:
        keys, off, locs, t2t = w["table"]
        w["dbs"][flags] = w["eng"].Database(keys, off, locs, t2t, flags=flags, **w["kw"])
    return w["dbs"][flags]


def _same(got, want, what):
    (gc, gn), (wc, wn) = got, want
    assert np.array_equal(gn, wn), (what, np.nonzero(gn != wn)[0][:8], gn[gn != wn][:8], wn[gn != wn][:8])
    mask = np.arange(gc.shape[1])[None, :] < wn[:, None]
    assert np.array_equal(gc[mask], wc[mask]), (what, np.nonzero((gc != wc).any(axis=2) & mask)[0][:8])


ROUTES = ["default", "MCQ_FORCE_RAW_SORT", "MCQ_NO_WAVE16", "MCQ_FORCE_BLOCK_PATH", "MCQ_DB_LOCS_64", "MCQ_DB_LOCS_GW"]


@pytest.mark.parametrize("tag,P", CASES)
@pytest.mark.parametrize("route", ROUTES)
def test_exclusion_is_the_filter_on_locations(tag, P, route):
    w = _world(tag, P)
    eng = w["eng"]
    db = _db(w, getattr(eng, route) if route.startswith("MCQ_DB_") else 0)
    flags = getattr(eng, route) if route.startswith("MCQ_FO") or route.startswith("MCQ_NO") else 0
    ws = eng.Workspace(db, w["nq"], len(w["bases"]))
    changed = 0
    for rank in (SPECIES, GENUS):
        ws.set_exclusion(w["tgt"][rank])
        for ranks in (1, P):
            for max_cand in (1, 4):
                ws.set_query_clades(w["qkey"][rank])
                got = ws.query_host(w["bases"], w["seq_off"], True, max_cand=max_cand, emulate_ranks=ranks, flags=flags)
                want = _expected(w, rank, max_cand, ranks)
                _same(got, want, (tag, P, route, rank, ranks, max_cand))
                keep = _expected(w, rank, max_cand, ranks, np.full(w["nq"], eng.MCQ_CLADE_KEEP_ALL, np.uint32))
                changed += int((want[1] != keep[1]).sum())
    assert changed > 0, "exclusion changes no list of this fixture: the comparison pins nothing"


@pytest.mark.parametrize("tag,P", [("mini", 4), ("noanc", 2)])
def test_keep_all_equals_no_exclusion(tag, P):
    """every query carries MCQ_CLADE_KEEP_ALL: byte-identical cands and n_cand to a workspace without exclusion"""
    w = _world(tag, P)
    eng = w["eng"]
    db = _db(w)
    plain = eng.Workspace(db, w["nq"], len(w["bases"]))
    ws = eng.Workspace(db, w["nq"], len(w["bases"]))
    ws.set_exclusion(w["tgt"][SPECIES])
    for flags in (0, eng.MCQ_QUIRK_SEQ_DROP):
        c0, n0 = plain.query_host(w["bases"], w["seq_off"], True, max_cand=w["fx"].maxcand, emulate_ranks=P, flags=flags)
        ws.set_query_clades(np.full(w["nq"], eng.MCQ_CLADE_KEEP_ALL, np.uint32))
        c1, n1 = ws.query_host(w["bases"], w["seq_off"], True, max_cand=w["fx"].maxcand, emulate_ranks=P, flags=flags)
        assert n0.tobytes() == n1.tobytes()
        mask = np.arange(c0.shape[1])[None, :] < n0[:, None]         # (slots beyond n_cand are not written by either)
        assert c0[mask].tobytes() == c1[mask].tobytes()
    ws.set_exclusion(None)                                            # detached: as ever, no keys needed
    c2, n2 = ws.query_host(w["bases"], w["seq_off"], True, max_cand=w["fx"].maxcand, emulate_ranks=P)
    assert n2.tobytes() == plain.query_host(w["bases"], w["seq_off"], True, max_cand=w["fx"].maxcand, emulate_ranks=P)[1].tobytes()


def test_all_hit_targets_excluded_gives_no_candidate():
    """a query whose hit targets all share one clade key, which is the query's: n_cand == 0"""
    w = _world("mini", 4)
    eng = w["eng"]
    ws = eng.Workspace(_db(w), w["nq"], len(w["bases"]))
    n_targets = len(w["tgt"][SPECIES])
    ws.set_exclusion(np.full(n_targets, 7, np.uint32))
    qk = np.full(w["nq"], eng.MCQ_CLADE_KEEP_ALL, np.uint32)
    hit = [q for q in range(w["nq"]) if len(w["matches"][q])]
    qk[hit[0]] = 7; qk[hit[-1]] = 7
    ws.set_query_clades(qk)
    _, n = ws.query_host(w["bases"], w["seq_off"], True, max_cand=4, emulate_ranks=4)
    assert n[hit[0]] == 0 and n[hit[-1]] == 0
    assert n[hit[1]] > 0


def test_missing_or_wrong_keys_are_argument_errors():
    w = _world("tie", 2)
    eng = w["eng"]
    ws = eng.Workspace(_db(w), w["nq"], len(w["bases"]))
    with pytest.raises(eng.McqError) as e:                            # no table attached: nothing to hand keys to
        ws.set_query_clades(w["qkey"][SPECIES])
    assert e.value.code == eng.MCQ_E_ARG
    ws.set_exclusion(w["tgt"][SPECIES])
    with pytest.raises(eng.McqError) as e:                            # attached, but no keys for the batch
        ws.query_host(w["bases"], w["seq_off"], True, max_cand=2, emulate_ranks=2)
    assert e.value.code == eng.MCQ_E_ARG
    ws.set_query_clades(w["qkey"][SPECIES][:-1])                      # one key short
    with pytest.raises(eng.McqError) as e:
        ws.query_host(w["bases"], w["seq_off"], True, max_cand=2, emulate_ranks=2)
    assert e.value.code == eng.MCQ_E_ARG
    ws.set_query_clades(w["qkey"][SPECIES])                           # consumed by ONE call
    ws.query_host(w["bases"], w["seq_off"], True, max_cand=2, emulate_ranks=2)
    with pytest.raises(eng.McqError) as e:
        ws.query_host(w["bases"], w["seq_off"], True, max_cand=2, emulate_ranks=2)
    assert e.value.code == eng.MCQ_E_ARG
    ws.set_query_clades(w["qkey"][SPECIES])
    with pytest.raises(eng.McqError) as e:                            # no lean first stage under exclusion
        ws.query_host(w["bases"], w["seq_off"], True, max_cand=2, emulate_ranks=2, flags=eng.MCQ_FORCE_LEAN_WAVE)
    assert e.value.code == eng.MCQ_E_UNSUPPORTED


def test_pipelined_batches_keep_their_own_keys():
    """two batches in flight, the same reads under different key arrays: each is answered with its own"""
    w = _world("mini", 4)
    eng = w["eng"]
    nq, M = w["nq"], 4
    ws = eng.Workspace(_db(w), nq, len(w["bases"]))
    ws.set_exclusion(w["tgt"][SPECIES])
    keep = np.full(nq, eng.MCQ_CLADE_KEEP_ALL, np.uint32)
    arrays = [w["qkey"][SPECIES], keep, w["qkey"][SPECIES]]
    bases = np.frombuffer(w["bases"], np.uint8).copy()
    seq_off = np.ascontiguousarray(w["seq_off"], np.uint64)
    outs, tickets = [], []
    for a in arrays:
        c = np.zeros((nq, M, 4), np.uint32)
        n = np.zeros(nq, np.uint32)
        scratch = a.copy()
        ws.set_query_clades(scratch)
        scratch[:] = 0                                                # the call has copied the host array
        tickets.append(ws.query_pipelined(bases.ctypes.data, seq_off.ctypes.data, 2 * nq, True, c.ctypes.data, n.ctypes.data,
                                          max_cand=M, emulate_ranks=4))
        outs.append((c, n))
    for t, (c, n), a in zip(tickets, outs, arrays):
        ws.wait(t)
        _same((c, n), _expected(w, SPECIES, M, 4, a), "pipelined")
    ws.sync()
