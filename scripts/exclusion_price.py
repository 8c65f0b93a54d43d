#!/usr/bin/env python3
"""The price of clade exclusion (mcq_ws_set_exclusion) on bench.py's default table (configs[1]: 50 species x 10 strains, 1 M reads
of 150 bases, emulate_ranks 2, max_cand 2): every read carries its source genome's species as its clade key, so its own species'
ten targets are retired.  Compared with the same forced route without exclusion -- the full first wave stage and no two-class
tail (MCQ_FORCE_FULL_WAVE | MCQ_NO_TWO_CLASS), which is where exclusion sends a batch.  Prints one JSON object: GPU milliseconds
per step (median of --reps after 3 warm-up steps, events around each call) and the mcq_stats counters of both.
usage: python scripts/exclusion_price.py [--small] [--out profiles/exclusion_price.json]"""
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
    db = eng.Database(None, None, None, None, device=0, device_ptrs=dict(keys=table.keys_ptr, list_off=table.list_off_ptr, locs=table.locs_ptr,
                      tgt2tax=sp32.data_ptr(), n_keys=table.n_keys, n_locs=table.n_locs, n_targets=n_targets))
    table.close()
    del gb
    ws = eng.Workspace(db, B, B * L)
    cands = torch.zeros((B, 2, 4), dtype=torch.int32, device=dev)
    ncand = torch.zeros(B, dtype=torch.int32, device=dev)
    tgt_clade = species.to(torch.int32).cpu().numpy().astype(np.uint32)            # a target's clade key: its species
    qkeys = species[src.to(dev)].to(torch.int32).contiguous()                      # a read's: its source genome's species
    flags = eng.MCQ_FORCE_FULL_WAVE | eng.MCQ_NO_TWO_CLASS
    st = torch.cuda.current_stream(dev).cuda_stream
    out = {"workload": "configs[1] table, %d species x 10 strains, %d reads x %d bases, emulate_ranks 2, max_cand 2, flags FULL_WAVE | NO_TWO_CLASS" % (n_species, B, L)}
    for name, excl in (("plain", False), ("exclusion", True)):
        ws.set_exclusion(tgt_clade if excl else None)
        ms = []
        for i in range(3 + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            if excl:
                ws.set_query_clades(None, device_ptr=qkeys.data_ptr(), n_queries=B)
            e0.record()
            ws.query_device(reads.data_ptr(), roff.data_ptr(), B, False, cands.data_ptr(), ncand.data_ptr(), max_cand=2, emulate_ranks=2,
                            flags=flags, stream=st)
            e1.record()
            e1.synchronize()
            if i >= 3:
                ms.append(e0.elapsed_time(e1))
        out[name] = {"ms_per_step": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms)), "stats": ws.sync(),
                     "queries_without_candidates": int((ncand == 0).sum().item())}
    out["ratio"] = out["exclusion"]["ms_per_step"] / out["plain"]["ms_per_step"]
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
