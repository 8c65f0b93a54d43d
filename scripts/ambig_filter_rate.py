#!/usr/bin/env python3
"""The time of mcq_table_remove_ambiguous (-remove-ambig-features on the device) on the table of bench.py's default genome set
(50 species x 10 strains of 2..6 Mbp, about 2 Gbp, emulate_ranks 2), beside the two existing operations of a build:
mcq_build_table, and mcq_table_rank_split (rank 0 of 2) -- the same traversal (a group of lanes per key, count, scans, scatter),
the yardstick.  The filter runs with the species of every target as its key, at N = 1 and N = 4.  Device-synchronised wall
time around each call, --reps alternating repeats in one process after one warm-up round of the three table operations.
Prints one JSON object: seconds per call (median, min, max), the ratios to the split, keys and locations before and after.
usage: python scripts/ambig_filter_rate.py [--small] [--out profiles/ambig_filter_rate.json]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="a tenth of the genome set (plumbing check)")
    a = ap.parse_args()
    import torch
    eng = importlib.import_module("metacache-mpi_amd.engine")
    synth = importlib.import_module("metacache-mpi_amd.synth")
    dev = torch.device("cuda", 0)
    n_species = 5 if a.small else 50
    gb, goff, species = synth.make_genomes(n_species, 10, 2_000_000, 6_000_000, 0.02, seed=1, device=dev)
    nt = species.numel()
    keys32 = species.to(torch.int32).contiguous()

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, r

    sec = {"build_table": [], "rank_split_0_of_2": [], "remove_ambiguous_n1": [], "remove_ambiguous_n4": []}
    sizes = {}
    for i in range(1 + a.reps):
        tb, table = timed(lambda: eng.Table(gb.data_ptr(), goff.data_ptr(), nt, emulate_ranks=2, device=0))
        ts, part = timed(lambda: table.rank_split(2, 0))
        t1, (f1, r1) = timed(lambda: table.remove_ambiguous(keys32.data_ptr(), 1))
        t4, (f4, r4) = timed(lambda: table.remove_ambiguous(keys32.data_ptr(), 4))
        sizes = {"table": {"keys": table.n_keys, "locations": table.n_locs}, "rank_0_of_2": {"keys": part.n_keys, "locations": part.n_locs},
                 "after_n1": {"keys": f1.n_keys, "locations": f1.n_locs, "removed": r1},
                 "after_n4": {"keys": f4.n_keys, "locations": f4.n_locs, "removed": r4}}
        for t in (part, f1, f4, table):
            t.close()
        if i >= 1:
            for k, v in zip(sec, (tb, ts, t1, t4)):
                sec[k].append(v)
    out = {"workload": "bench.py default genome set: %d species x 10 strains, %d targets, %d bases, emulate_ranks 2; keys: the species of every target"
                       % (n_species, nt, int(goff[-1].item())), "reps": a.reps, "timer": "wall time between device synchronisations, seconds"}
    for k, v in sec.items():
        out[k] = {"s_per_call": float(np.median(v)), "s_min": float(min(v)), "s_max": float(max(v))}
    for k in ("remove_ambiguous_n1", "remove_ambiguous_n4"):
        out[k]["ratio_to_rank_split"] = out[k]["s_per_call"] / out["rank_split_0_of_2"]["s_per_call"]
    out["sizes"] = sizes
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
