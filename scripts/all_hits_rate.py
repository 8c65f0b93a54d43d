#!/usr/bin/env python3
"""The price of mcq_all_hits_count + mcq_all_hits (the kernels behind -allhits) on bench.py's default table (configs[1]: 50 species
x 10 strains, 1 M reads of 150 bases, emulate_ranks 2, max_cand 2).  Both calls redo rows 1-7 of every read, so the yardstick is the
query step of the same library in the same session on the same handle.  The entry buffer is sized once from the first count.
Prints one JSON object: GPU milliseconds per call (median of --reps after 3 warm-up calls, events around each call, the calls of
the three kinds alternating), count + emit per 1 Mi reads, its ratio to the query step, and what the kernels answered.
usage: python scripts/all_hits_rate.py [--small] [--out profiles/all_hits_rate.json]"""
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
    table = eng.Table(gb.data_ptr(), goff.data_ptr(), n_targets, emulate_ranks=2, device=0)
    ptrs = dict(keys=table.keys_ptr, list_off=table.list_off_ptr, locs=table.locs_ptr, n_keys=table.n_keys, n_locs=table.n_locs, n_targets=n_targets)
    db = eng.Database(None, None, None, None, device=0, device_ptrs=dict(ptrs, tgt2tax=sp32.data_ptr()))
    table.close()
    del gb
    ws = eng.Workspace(db, B, B * L)
    st = torch.cuda.current_stream(dev).cuda_stream
    cands = torch.zeros((B, 2, 4), dtype=torch.int32, device=dev)
    ncand = torch.zeros(B, dtype=torch.int32, device=dev)
    loc_off = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    n_hits = torch.zeros(B, dtype=torch.int32, device=dev)
    status = torch.zeros(B, dtype=torch.int32, device=dev)

    def query():
        ws.query_device(reads.data_ptr(), roff.data_ptr(), B, False, cands.data_ptr(), ncand.data_ptr(), max_cand=2, emulate_ranks=2, stream=st)

    def count():
        ws.all_hits_count(reads.data_ptr(), roff.data_ptr(), B, False, loc_off.data_ptr(), stream=st)

    count()
    torch.cuda.synchronize(dev)
    total = int(loc_off[B].item())
    hits = torch.zeros((max(total, 1), 3), dtype=torch.int32, device=dev)

    def emit():
        ws.all_hits(reads.data_ptr(), roff.data_ptr(), B, False, loc_off.data_ptr(), hits.data_ptr(), total, n_hits.data_ptr(),
                    status.data_ptr(), stream=st)

    calls = {"query": query, "all_hits_count": count, "all_hits": emit}
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
    ws.sync(st)
    nh = n_hits.cpu().numpy().view(np.uint32).astype(np.int64)
    out = {"workload": "configs[1] table, %d species x 10 strains, %d reads x %d bases, emulate_ranks 2, max_cand 2" % (n_species, B, L),
           "reps": a.reps}
    for k, v in ms.items():
        out[k] = {"ms_per_call": float(np.median(v)), "ms_min": float(min(v)), "ms_max": float(max(v))}
    both = out["all_hits_count"]["ms_per_call"] + out["all_hits"]["ms_per_call"]
    out["count_plus_emit_ms_per_1Mi_reads"] = both * (1 << 20) / B
    out["ratio_to_query_step"] = both / out["query"]["ms_per_call"]
    out["answered"] = {"locations": total, "entries": int(nh.sum()), "entry_buffer_MB": total * 12 / 1e6,
                       "longest_segment": int(np.diff(loc_off.cpu().numpy()).max()), "queries_with_a_status": int((status != 0).sum().item())}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
