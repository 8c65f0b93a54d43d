#!/usr/bin/env python3
"""The price of mcq_target_hits (the kernel behind -hits-per-seq) on bench.py's default table (configs[1]: 50 species x 10 strains,
1 M reads of 150 bases, emulate_ranks 2, max_cand 2), n_slots 2.  The slot targets come from the batch's own results: the table is
queried once with sequence-level taxon keys (one key per target) and mcq_target_slots turns the two candidates of every read
into its slots.  mcq_target_hits redoes rows 1-7 of the read, so the yardstick is the query step of the same library in the same
session, on the handle bench.py times (species-level keys); the query step at sequence level is reported beside it.
Prints one JSON object: GPU milliseconds per call (median of --reps after 3 warm-up calls, events around each call, the calls
of the three kinds alternating), the ratio, and what the kernel answered.
usage: python scripts/target_hits_rate.py [--small] [--out profiles/target_hits_rate.json]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--small", action="store_true", help="a tenth of the table and of the batch (plumbing check)")
    a = ap.parse_args()
    import torch
    eng = importlib.import_module("metacache-mpi_amd.engine")
    synth = importlib.import_module("metacache-mpi_amd.synth")
    dev = torch.device("cuda", 0)
    n_species, B, L = (5, 100_000, 150) if a.small else (50, 1 << 20, 150)
    gb, goff, species = synth.make_genomes(n_species, 10, 2_000_000, 6_000_000, 0.02, seed=1, device=dev)
    n_targets = species.numel()
    reads, roff, src = synth.sample_reads(gb, goff, B, L, 0.005, 0.001, seed=1000)
    sp32 = species.to(torch.int32).contiguous()
    seq32 = (torch.arange(n_targets, device=dev, dtype=torch.int64) - (1 << 31)).to(torch.int32).contiguous()     # 0x80000000 | target
    table = eng.Table(gb.data_ptr(), goff.data_ptr(), n_targets, emulate_ranks=2, device=0)
    ptrs = dict(keys=table.keys_ptr, list_off=table.list_off_ptr, locs=table.locs_ptr, n_keys=table.n_keys, n_locs=table.n_locs, n_targets=n_targets)
    db_sp = eng.Database(None, None, None, None, device=0, device_ptrs=dict(ptrs, tgt2tax=sp32.data_ptr()))
    db_seq = eng.Database(None, None, None, None, device=0, device_ptrs=dict(ptrs, tgt2tax=seq32.data_ptr()))
    table.close()
    del gb
    ws_sp, ws_seq = eng.Workspace(db_sp, B, B * L), eng.Workspace(db_seq, B, B * L)
    st = torch.cuda.current_stream(dev).cuda_stream
    n_slots = 2
    cands = torch.zeros((B, 2, 4), dtype=torch.int32, device=dev)
    ncand = torch.zeros(B, dtype=torch.int32, device=dev)
    tax2tgt = torch.arange(n_targets, device=dev, dtype=torch.int32)               # the keys of db_seq are 0x80000000 | target
    slots = torch.zeros((B, n_slots), dtype=torch.int32, device=dev)
    cap = ws_seq.target_hits_range_cap(L)
    rng = torch.zeros((B, n_slots, 4), dtype=torch.int32, device=dev)
    cnt = torch.zeros((B, n_slots, cap), dtype=torch.int32, device=dev)
    status = torch.zeros(B, dtype=torch.int32, device=dev)

    def q_species():
        ws_sp.query_device(reads.data_ptr(), roff.data_ptr(), B, False, cands.data_ptr(), ncand.data_ptr(), max_cand=2, emulate_ranks=2, stream=st)

    def q_sequence():
        ws_seq.query_device(reads.data_ptr(), roff.data_ptr(), B, False, cands.data_ptr(), ncand.data_ptr(), max_cand=2, emulate_ranks=2, stream=st)

    def hits():
        ws_seq.target_hits(reads.data_ptr(), roff.data_ptr(), B, False, slots.data_ptr(), n_slots, cap, rng.data_ptr(), cnt.data_ptr(),
                           status.data_ptr(), stream=st)

    q_sequence()
    eng.target_slots(cands.data_ptr(), ncand.data_ptr(), B, 2, 1, tax2tgt.data_ptr(), n_targets, slots.data_ptr(), n_slots, stream=st)
    torch.cuda.synchronize(dev)
    calls = {"query_species_keys": q_species, "query_sequence_keys": q_sequence, "target_hits": hits}
    ms = {k: [] for k in calls}
    for i in range(3 + a.reps):
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= 3:
                ms[name].append(e0.elapsed_time(e1))
    ws_seq.sync(st)                                                               # (raises if a read was beyond the kernel's capacity)
    r = rng.cpu().numpy().view(np.uint32)
    used = r[:, :, 0] != 0xFFFFFFFF
    out = {"workload": "configs[1] table, %d species x 10 strains, %d reads x %d bases, emulate_ranks 2, max_cand 2; n_slots %d, range_cap %d"
                       % (n_species, B, L, n_slots, cap),
           "reps": a.reps}
    for k, v in ms.items():
        out[k] = {"ms_per_call": float(np.median(v)), "ms_min": float(min(v)), "ms_max": float(max(v))}
    out["ms_per_1M_reads"] = out["target_hits"]["ms_per_call"] * (1 << 20) / B
    out["ratio_to_query_step"] = out["target_hits"]["ms_per_call"] / out["query_species_keys"]["ms_per_call"]
    out["answered"] = {"slots_used": int(used.sum()), "slots_with_a_range": int((r[:, :, 3] > 0).sum()), "hits_in_ranges": int(r[:, :, 1].sum()),
                       "queries_beyond_capacity": int((status != 0).sum().item())}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
