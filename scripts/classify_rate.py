#!/usr/bin/env python3
"""Time mcq_classify (k_classify: classification + per-taxon counts) on the taxonomy of bench.py's default table (configs[1]:
50 species x 10 strains, a root, the 500 targets as sequence-level taxa) at 1 M and 8 M queries, max_cand 2 and 4, with
every query's top candidate on one taxon ("one") or spread over all 551 taxa, species and sequence-level keys ("spread").
Candidate lists as the query kernels write them: a second candidate on a sister taxon with fewer hits half of the time.
Prints one JSON object (GPU milliseconds per call, median of 20 after 3 warm-up calls, CUDA events around each call).
usage: python scripts/classify_rate.py [--out profiles/classify_rate.json]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def taxonomy(n_species=50, strains=10):
    """index 0 root (rank 20), 1..n_species species (rank 4), then the targets (rank 0) under their species"""
    n = 1 + n_species + n_species * strains
    NO = 0xFFFFFFFF
    lin = np.full((n, 21), NO, np.uint32); rank = np.zeros(n, np.uint8)
    lin[:, 20] = 0; rank[0] = 20
    for s in range(n_species):
        i = 1 + s
        rank[i] = 4; lin[i, 4] = i
        for t in range(strains):
            j = 1 + n_species + s * strains + t
            lin[j, 4] = i; lin[j, 0] = j
    return lin, rank


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import torch
    eng = importlib.import_module("metacache-mpi_amd.engine")
    lin, rank = taxonomy()
    nt = len(rank)
    tx = eng.Taxonomy(lin, rank)
    rng = np.random.default_rng(1)
    res = {"taxa": nt, "results": []}
    for n in (1 << 20, 8 << 20):
        for max_cand in (2, 4):
            for dist in ("one", "spread"):
                c = np.zeros((n, max_cand, 4), np.uint32)
                top = np.full(n, 1, np.uint32) if dist == "one" else rng.integers(1, nt, n).astype(np.uint32)
                seq = top > 50
                c[:, 0, 0] = np.where(seq, top | 0x80000000, top)
                h0 = rng.integers(4, 40, n).astype(np.uint32)
                c[:, 0, 1] = h0
                second = rng.random(n) < 0.5
                sib = np.where(seq, ((top - 51 + 1) % 500 + 51) | 0x80000000, top % 50 + 1).astype(np.uint32)
                c[:, 1, 0] = np.where(second, sib, 0); c[:, 1, 1] = np.where(second, np.maximum(h0 - rng.integers(0, 8, n), 1), 0)
                ncand = np.where(second, 2, 1).astype(np.uint32)
                dc = torch.from_numpy(c.view(np.int32)).cuda(); dn = torch.from_numpy(ncand.view(np.int32)).cuda()
                counts = torch.zeros(nt + 1, dtype=torch.int64, device="cuda")
                times = []
                for r in range(3 + a.reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    tx.classify(dc.data_ptr(), dn.data_ptr(), n, max_cand, 4, 0.8, 19, None, counts.data_ptr())
                    e1.record()
                    torch.cuda.synchronize()
                    if r >= 3:
                        times.append(e0.elapsed_time(e1))
                got = counts.cpu().numpy()
                assert got.sum() == n * (3 + a.reps), "counts lost"
                ms = float(np.median(times))
                res["results"].append({"n_queries": n, "max_cand": max_cand, "distribution": dist, "ms": ms,
                                       "us_per_1M_queries": ms * 1e3 / (n / 2 ** 20), "candidate_GBps": n * max_cand * 16 / ms / 1e6})
                print(json.dumps(res["results"][-1]), file=sys.stderr)
                del dc, dn
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
