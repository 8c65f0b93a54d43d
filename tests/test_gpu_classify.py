"""Classification and per-taxon counts on the device (mcq_classify, mcq_ws_set_classify / mcq_ws_taxon_counts) against the
host classification (mcq_refdb_classify) and a Python restatement of classify (src/classification.cpp:235-265)."""
import importlib

import numpy as np
import pytest

from golden_util import Fixture
from oracle import dbfile
from oracle import mc_oracle as orc

pytestmark = pytest.mark.gpu
NO = 0xFFFFFFFF
F32 = np.float32


@pytest.fixture(scope="module")
def env():
    import torch
    eng = importlib.import_module("metacache-mpi_amd.engine")
    host = importlib.import_module("metacache-mpi_amd.host")
    return torch, eng, host


def _fixture_db(eng, host, tag, P):
    fx = Fixture(tag, P)
    keys, off, locs = dbfile.union_shards(fx.shards)
    p = fx.params
    db = eng.Database(keys, off, locs, fx.tgt2tax(), sketch_size=p["qs"], k=p["qk"], winlen=p["qwinlen"],
                      winstride=p["qwinstride"], tgt_winstride=p["winstride"])
    rdb = host.RefDb(fx.shard_paths[0][: -len(".db_0")], P)
    return fx, db, rdb


def _device_query(torch, eng, fx, db):
    bases, seq_off = orc.pack_reads(fx.interleaved())
    n = len(fx.names)
    ws = eng.Workspace(db, max_queries=n, max_bases=len(bases))
    d_b = torch.from_numpy(np.frombuffer(bases, np.uint8).copy()).cuda()
    d_o = torch.from_numpy(seq_off.astype(np.int64)).cuda()
    cands = torch.zeros((n, fx.maxcand, 4), dtype=torch.int32, device="cuda")
    ncand = torch.zeros(n, dtype=torch.int32, device="cuda")
    ws.query_device(d_b.data_ptr(), d_o.data_ptr(), 2 * n, True, cands.data_ptr(), ncand.data_ptr(), max_cand=fx.maxcand,
                    emulate_ranks=fx.P, flags=eng.MCQ_QUIRK_SEQ_DROP)
    ws.sync()
    return ws, cands, ncand, (d_b, d_o, bases, seq_off)


def _classify_dev(torch, eng, tx, cands, ncand, n, max_cand, hits_min, frac, highest, counts=True):
    best = torch.zeros(max(n, 1), dtype=torch.int32, device="cuda")
    cnt = torch.zeros(tx.n_taxa + 1, dtype=torch.int64, device="cuda") if counts else None
    tx.classify(cands.data_ptr(), ncand.data_ptr(), n, max_cand, hits_min, frac, highest, best.data_ptr(),
                cnt.data_ptr() if counts else None)
    torch.cuda.synchronize()
    return best.cpu().numpy().view(np.uint32)[:n], (cnt.cpu().numpy().view(np.uint64) if counts else None)


@pytest.mark.parametrize("tag,P", [("mini", 4), ("tie", 2), ("noanc", 2), ("wide", 16)])
def test_device_classification_equals_the_host_one(env, tag, P):
    torch, eng, host = env
    fx, db, rdb = _fixture_db(eng, host, tag, P)
    ws, cands, ncand, _ = _device_query(torch, eng, fx, db)
    tx = eng.Taxonomy(*rdb.lineages())
    hc = cands.cpu().numpy().view(np.uint32); hn = ncand.cpu().numpy().view(np.uint32)
    n = len(fx.names)
    default = int(host.lib().mcq_default_hits_min(fx.params["qs"]))
    for frac in (0.333, 0.8, 0.95, 1.0):
        for hits_min in (1, 4, default):
            for highest in (4, 6, 20):
                best, counts = _classify_dev(torch, eng, tx, cands, ncand, n, fx.maxcand, hits_min, frac, highest)
                want = np.array([rdb.classify(hc[q, :hn[q]], hits_min, float(F32(frac)), highest) for q in range(n)], np.uint32)
                assert np.array_equal(best, want), (frac, hits_min, highest)
                key = np.where(want == NO, tx.n_taxa, want)
                assert np.array_equal(counts, np.bincount(key, minlength=tx.n_taxa + 1).astype(np.uint64))


# ---- synthetic ------------------------------------------------------------------------------------------------------------
def _deep_taxonomy(rng, n_taxa):
    """random tree: taxon i > 0 hangs below a random earlier taxon of higher rank; some ranks are skipped (missing ranks)"""
    parent = np.zeros(n_taxa, np.int64); rank = np.zeros(n_taxa, np.uint8)
    rank[0] = 20
    for i in range(1, n_taxa):
        p = int(rng.integers(0, i))
        while rank[p] == 0:
            p = int(parent[p])
        parent[i] = p
        rank[i] = int(rng.integers(0, rank[p]))
    lin = np.full((n_taxa, 21), NO, np.uint32)
    for i in range(n_taxa):
        c = i
        while True:
            lin[i, rank[c]] = c
            if c == 0:
                break
            c = int(parent[c])
    return lin, rank


def _restated_classify(lin, rank, c, n, hits_min, frac, highest):
    """mcq_refdb_classify restated: c = [(tax, hits)]"""
    nt = len(rank)
    valid = lambda k: k != NO and (k & 0x7FFFFFFF) < nt
    if n == 0 or not valid(int(c[0][0])):
        return NO
    h0 = int(c[0][1])
    if h0 < hits_min:
        return NO
    lca = int(c[0][0]) & 0x7FFFFFFF
    thr = F32(F32(h0 - hits_min) * F32(frac)) if h0 > hits_min else F32(0)
    for i in range(1, n):
        if not (F32(int(c[i][1])) > thr):
            break
        r = NO
        k = int(c[i][0])
        if valid(k):
            b = k & 0x7FFFFFFF
            for j in range(21):
                x = int(lin[lca, j])
                if x != NO and x == int(lin[b, j]):
                    r = x
                    break
        lca = r
        if lca == NO or rank[lca] > highest:
            return NO
    return lca if rank[lca] <= highest else NO


def _pool(rng, lin, rank, max_cand, n_pool, hits_min):
    """n_pool random candidate lists with every corner: bit-31 keys, keys past the table, 0xFFFFFFFF, empty lists, hits at
    hits_min and at the threshold's edge"""
    nt = len(rank)
    c = np.zeros((n_pool, max_cand, 4), np.uint32)
    nc = rng.integers(0, max_cand + 1, n_pool).astype(np.uint32)
    tax = rng.integers(0, nt, (n_pool, max_cand)).astype(np.uint32)
    u = rng.random((n_pool, max_cand))
    tax[u < 0.10] |= 0x80000000
    tax[(u >= 0.10) & (u < 0.13)] = NO
    tax[(u >= 0.13) & (u < 0.15)] = nt + rng.integers(0, 5)
    h0 = rng.integers(0, 30, n_pool)
    h0[rng.random(n_pool) < 0.1] = hits_min
    hits = np.sort(rng.integers(0, 30, (n_pool, max_cand)), axis=1)[:, ::-1].copy()
    hits[:, 0] = np.maximum(hits[:, 0], h0)
    hits = np.minimum(hits, hits[:, :1])
    c[:, :, 0] = tax; c[:, :, 1] = hits
    return c, nc


@pytest.mark.parametrize("max_cand", list(range(1, 17)))
def test_random_lists_against_the_restatement(env, max_cand):
    torch, eng, host = env
    rng = np.random.default_rng(100 + max_cand)
    lin, rank = _deep_taxonomy(rng, 3000)
    tx = eng.Taxonomy(lin, rank)
    for (hits_min, frac, highest) in ((1, 0.8, 19), (4, 0.333, 20), (2, 1.0, 6)):
        pc, pn = _pool(rng, lin, rank, max_cand, 2048, hits_min)
        want_pool = np.array([_restated_classify(lin, rank, pc[i, :, :2], pn[i], hits_min, frac, highest) for i in range(len(pn))], np.uint32)
        sizes = (1, 63, 64, 65, 1 << 20, 3 << 20) if max_cand in (1, 4, 16) else (1, 63, 64, 65, 4099)
        for n in sizes:
            idx = rng.integers(0, len(pn), n) if n > 65 else np.arange(n)
            dc = torch.from_numpy(pc[idx].view(np.int32)).cuda(); dn = torch.from_numpy(pn[idx].view(np.int32)).cuda()
            best, counts = _classify_dev(torch, eng, tx, dc, dn, n, max_cand, hits_min, frac, highest)
            want = want_pool[idx]
            assert np.array_equal(best, want), (max_cand, n, hits_min, frac, highest)
            key = np.where(want == NO, tx.n_taxa, want)
            assert np.array_equal(counts, np.bincount(key, minlength=tx.n_taxa + 1).astype(np.uint64)), (max_cand, n)
            # counts only (no best output): the same counts
            b2 = torch.zeros(tx.n_taxa + 1, dtype=torch.int64, device="cuda")
            tx.classify(dc.data_ptr(), dn.data_ptr(), n, max_cand, hits_min, frac, highest, None, b2.data_ptr())
            torch.cuda.synchronize()
            assert np.array_equal(b2.cpu().numpy().view(np.uint64), counts)
            del dc, dn


def test_skewed_counts_are_exact(env):
    """2 M queries on one taxon plus 1 M spread over 100 k taxa: exact integer counts (the one taxon goes through the
    workgroup tables, the spread ones overflow them into direct atomics)"""
    torch, eng, host = env
    nt = 100_001
    lin = np.full((nt, 21), NO, np.uint32); lin[:, 4] = np.arange(nt); rank = np.full(nt, 4, np.uint8)
    tx = eng.Taxonomy(lin, rank)
    rng = np.random.default_rng(3)
    tax = np.concatenate([np.full(2 << 20, 7, np.uint32), rng.integers(0, 100_000, 1 << 20).astype(np.uint32)])
    rng.shuffle(tax)
    n = len(tax)
    for max_cand in (2, 4):
        c = np.zeros((n, max_cand, 4), np.uint32); c[:, 0, 0] = tax; c[:, 0, 1] = 10
        dc = torch.from_numpy(c.view(np.int32)).cuda(); dn = torch.ones(n, dtype=torch.int32, device="cuda")
        best, counts = _classify_dev(torch, eng, tx, dc, dn, n, max_cand, 4, 0.8, 19)
        assert np.array_equal(best, tax)
        assert np.array_equal(counts, np.bincount(tax, minlength=nt + 1).astype(np.uint64))
        assert counts[7] >= (2 << 20)
        del dc, dn


def test_workspace_counts_follow_the_attached_taxonomy(env):
    """mcq_query_pipelined over several batches with a taxonomy attached: the workspace's counts equal the host
    classifications; detached, nothing accumulates; reset zeroes them"""
    torch, eng, host = env
    fx, db, rdb = _fixture_db(eng, host, "mini", 4)
    tx = eng.Taxonomy(*rdb.lineages())
    seqs = fx.interleaved()
    n = len(fx.names)
    ws = eng.Workspace(db, max_queries=n, max_bases=sum(len(s) for s in seqs))
    with pytest.raises(eng.McqError):
        ws.taxon_counts()                                  # nothing attached yet
    ws.set_classify(tx, fx.hitmin, fx.hitdiff, fx.highest)
    cuts = [0, 50, 51, 120, n]
    keep, want = [], np.zeros(tx.n_taxa + 1, np.uint64)
    tickets = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        bases, off = orc.pack_reads(seqs[2 * a: 2 * b])
        bb = np.frombuffer(bases, np.uint8).copy()
        cc = np.zeros((b - a, fx.maxcand, 4), np.uint32); nn = np.zeros(b - a, np.uint32)
        keep.append((bb, off, cc, nn))
        tickets.append(ws.query_pipelined(bb.ctypes.data, off.ctypes.data, 2 * (b - a), True, cc.ctypes.data, nn.ctypes.data,
                                          max_cand=fx.maxcand, emulate_ranks=fx.P, flags=eng.MCQ_QUIRK_SEQ_DROP))
    for t, (bb, off, cc, nn) in zip(tickets, keep):
        ws.wait(t)
        for q in range(len(nn)):
            k = rdb.classify(cc[q, :nn[q]], fx.hitmin, fx.hitdiff, fx.highest)
            want[tx.n_taxa if k == NO else k] += 1
    got = ws.taxon_counts()
    assert np.array_equal(got, want) and got.sum() == n
    # the synchronous call adds too
    bases, off = orc.pack_reads(seqs)
    ws.query_host(bases, off, True, max_cand=fx.maxcand, emulate_ranks=fx.P, flags=eng.MCQ_QUIRK_SEQ_DROP)
    assert np.array_equal(ws.taxon_counts(), 2 * want)
    ws.set_classify(None)
    ws.query_host(bases, off, True, max_cand=fx.maxcand, emulate_ranks=fx.P, flags=eng.MCQ_QUIRK_SEQ_DROP)
    assert np.array_equal(ws.taxon_counts(reset=True), 2 * want)
    assert not ws.taxon_counts().any()


def test_sharded_results_give_the_fused_counts(env):
    """eng.Shard at one rank: mcq_classify on its device result equals the counts of the fused path"""
    torch, eng, host = env
    fx, db, rdb = _fixture_db(eng, host, "mini", 4)
    tx = eng.Taxonomy(*rdb.lineages())
    ws, cands, ncand, (d_b, d_o, bases, seq_off) = _device_query(torch, eng, fx, db)
    n = len(fx.names)
    _, fused = _classify_dev(torch, eng, tx, cands, ncand, n, fx.maxcand, fx.hitmin, fx.hitdiff, fx.highest)
    sh = eng.Shard(db, 1, 0, max_queries=n, max_bases=len(bases) + 64, max_seqs=2 * n)
    c2 = torch.zeros((n, fx.maxcand, 4), dtype=torch.int32, device="cuda"); n2 = torch.zeros(n, dtype=torch.int32, device="cuda")
    sh.query(d_b.data_ptr(), d_o.data_ptr(), 2 * n, True, c2.data_ptr(), n2.data_ptr(), max_cand=fx.maxcand, emulate_ranks=fx.P,
             flags=eng.MCQ_QUIRK_SEQ_DROP)
    sh.sync()
    _, sharded = _classify_dev(torch, eng, tx, c2, n2, n, fx.maxcand, fx.hitmin, fx.hitdiff, fx.highest)
    assert np.array_equal(sharded, fused) and fused.sum() == n
