"""The harness of tests/test_gpu_all_hits.py around Workspace.all_hits_count / all_hits: guard entries in front of and behind the entry
array, a fill word in everything the call may not touch, and offsets or a capacity of the test's own in place of the counted ones."""
import numpy as np

from all_hits_ref import HIT

FILL = 0xA5A5A5A5


def all_hits_guarded(ws, bases, seq_off, paired, packed=False, ranges=False, guard=16, cap=None, loc_off=None):
    """numpy in, numpy out (the copies go through torch; waits for the device).  Returns a dict: loc_off u64 [nq + 1] as
    mcq_all_hits_count left it, n_hits / status u32 [nq], hits: per query its entries (HIT records), raw: the whole entry array as u32
    words with `guard` entries of FILL words in front of and behind it (what the call left alone still holds FILL), total: entries
    between the guards.  cap None: loc_off[nq].  loc_off: offsets to use in place of the counted ones."""
    import torch
    dev = torch.device("cuda", ws.db.device)
    seq_off = np.ascontiguousarray(seq_off, np.uint64)
    n_seqs = len(seq_off) // 2 if ranges else len(seq_off) - 1
    nq = n_seqs // 2 if paired else n_seqs
    raw = np.frombuffer(bases, dtype=np.uint8) if not isinstance(bases, np.ndarray) else bases.view(np.uint8)
    d_bases = torch.from_numpy(np.concatenate([raw, np.zeros(8, np.uint8)])).to(dev)
    d_seq = torch.from_numpy(seq_off.view(np.int64)).to(dev) if len(seq_off) else torch.zeros(1, dtype=torch.int64, device=dev)
    pb = int(seq_off[-1]) if packed else 0
    st = torch.cuda.current_stream(dev).cuda_stream
    d_off = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
    ws.all_hits_count(d_bases.data_ptr(), d_seq.data_ptr(), n_seqs, paired, d_off.data_ptr(), stream=st, ranges=ranges, packed_bases=pb)
    torch.cuda.synchronize(dev)
    counted = d_off.cpu().numpy().view(np.uint64).copy()
    use = counted if loc_off is None else np.ascontiguousarray(loc_off, np.uint64)
    if loc_off is not None:
        d_off = torch.from_numpy(use.view(np.int64)).to(dev)
    total = int(max(int(use.max()), int(counted[nq]))) if nq else 0
    if cap is None:
        cap = int(counted[nq])
    h_hits = np.full(3 * (total + 2 * guard) + 3, FILL, np.uint32)
    d_hits = torch.from_numpy(h_hits.view(np.int32)).to(dev)
    d_n = torch.from_numpy(np.full(max(nq, 1) + 4, FILL, np.uint32).view(np.int32)).to(dev)
    d_st = torch.from_numpy(np.full(max(nq, 1) + 4, FILL, np.uint32).view(np.int32)).to(dev)
    ws.all_hits(d_bases.data_ptr(), d_seq.data_ptr(), n_seqs, paired, d_off.data_ptr(), d_hits.data_ptr() + 12 * guard, cap,
                d_n.data_ptr(), d_st.data_ptr(), stream=st, ranges=ranges, packed_bases=pb)
    torch.cuda.synchronize(dev)
    words = d_hits.cpu().numpy().view(np.uint32)
    n_all, st_all = d_n.cpu().numpy().view(np.uint32), d_st.cpu().numpy().view(np.uint32)
    assert (n_all[nq:] == FILL).all() and (st_all[nq:] == FILL).all(), "mcq_all_hits wrote behind n_hits or status"
    n_hits, status = n_all[:nq].copy(), st_all[:nq].copy()
    ent = words[3 * guard:3 * (guard + total)].view(HIT) if total else np.zeros(0, HIT)
    hits = [ent[int(use[q]):int(use[q]) + int(n_hits[q])].copy() for q in range(nq)]
    return {"loc_off": counted, "n_hits": n_hits, "status": status, "hits": hits, "raw": words, "fill": FILL, "guard": guard, "total": total}
