#!/usr/bin/env python3
"""The price of mcq_align (the kernel behind -align): 1 Mi read pairs of 2 x 150 bases, each aligned against a subject of four
target windows (3 x 113 + 128 = 467 bases) that contains both mates -- the job -align makes of a classified pair at -lowest
sequence.  The subjects are slices of bench.py's default genomes (configs[1]: 50 species x 10 strains); mate 1 is a copy of 150
bases of its subject with 1 % substitutions, mate 2 the reverse complement of another 150; every second pair is turned round, so
both orientations win.  The yardstick is the query step of the same library in the same session on bench.py's default table and
reads (1 Mi reads of 150 bases, emulate_ranks 2, max_cand 2).
Prints one JSON object: GPU milliseconds per call (median of --reps after 2 warm-up calls, events around each call, the two kinds
alternating), the ratio, and what the kernel answered.
usage: python scripts/align_rate.py [--small] [--out profiles/align_rate.json]"""
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="a tenth of the table and of the batch (plumbing check)")
    a = ap.parse_args()
    import torch
    eng = importlib.import_module("metacache-mpi_amd.engine")
    synth = importlib.import_module("metacache-mpi_amd.synth")
    dev = torch.device("cuda", 0)
    n_species, B, L, S = (5, 100_000, 150, 467) if a.small else (50, 1 << 20, 150, 467)
    gb, goff, species = synth.make_genomes(n_species, 10, 2_000_000, 6_000_000, 0.02, seed=1, device=dev)
    n_targets = species.numel()
    reads, roff, src = synth.sample_reads(gb, goff, B, L, 0.005, 0.001, seed=1000)
    sp32 = species.to(torch.int32).contiguous()
    table = eng.Table(gb.data_ptr(), goff.data_ptr(), n_targets, emulate_ranks=2, device=0)
    ptrs = dict(keys=table.keys_ptr, list_off=table.list_off_ptr, locs=table.locs_ptr, n_keys=table.n_keys, n_locs=table.n_locs, n_targets=n_targets)
    db = eng.Database(None, None, None, None, device=0, device_ptrs=dict(ptrs, tgt2tax=sp32.data_ptr()))
    table.close()
    ws = eng.Workspace(db, B, 2 * B * L)
    st = torch.cuda.current_stream(dev).cuda_stream
    # ---- the pairs and their subjects
    g = torch.Generator(device=dev); g.manual_seed(7)
    n_bases = gb.numel()
    sub_off = torch.randint(0, n_bases - S, (B,), device=dev, generator=g, dtype=torch.int64)
    a1 = torch.randint(0, S - L + 1, (B,), device=dev, generator=g, dtype=torch.int64)
    a2 = torch.randint(0, S - L + 1, (B,), device=dev, generator=g, dtype=torch.int64)
    idx = torch.arange(L, device=dev, dtype=torch.int64)
    comp = torch.arange(256, device=dev, dtype=torch.int64)
    for x, y in zip(b"ACGTacgt", b"TGCAtgca"):
        comp[x] = y
    acgt = torch.tensor(list(b"ACGT"), device=dev, dtype=torch.uint8)

    def noisy(m):
        hit = torch.rand(m.shape, device=dev, generator=g) < 0.01
        return torch.where(hit, acgt[torch.randint(0, 4, m.shape, device=dev, generator=g)], m)

    def rc(m):
        return comp[m.flip(1).to(torch.int64)].to(torch.uint8)

    m1 = noisy(gb[(sub_off + a1)[:, None] + idx[None, :]])
    m2 = rc(noisy(gb[(sub_off + a2)[:, None] + idx[None, :]]))
    turn = (torch.arange(B, device=dev) % 2 == 1)[:, None]
    m1, m2 = torch.where(turn, rc(m1), m1), torch.where(turn, rc(m2), m2)
    pairs = torch.stack([m1, m2], 1).contiguous().view(-1)                     # mates of pair q: sequences 2q, 2q + 1
    poff = (torch.arange(2 * B + 1, device=dev, dtype=torch.int64) * L).contiguous()
    jobs = torch.stack([sub_off, torch.full((B,), S | (1 << 32), device=dev, dtype=torch.int64)], 1).contiguous()   # mcq_align_job
    text_cap = L + S
    res = torch.zeros((B, 4), dtype=torch.int32, device=dev)
    out_q = torch.zeros(B * text_cap, dtype=torch.uint8, device=dev)
    out_s = torch.zeros(B * text_cap, dtype=torch.uint8, device=dev)
    cands = torch.zeros((B, 2, 4), dtype=torch.int32, device=dev)
    ncand = torch.zeros(B, dtype=torch.int32, device=dev)

    def query():
        ws.query_device(reads.data_ptr(), roff.data_ptr(), B, False, cands.data_ptr(), ncand.data_ptr(), max_cand=2, emulate_ranks=2, stream=st)

    def align():
        ws.align_device(pairs.data_ptr(), poff.data_ptr(), 2 * B, True, gb.data_ptr(), jobs.data_ptr(), L, S, res.data_ptr(),
                        out_q.data_ptr(), out_s.data_ptr(), text_cap, stream=st)

    calls = {"query_step": query, "align": align}
    ms = {k: [] for k in calls}
    for i in range(2 + a.reps):
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= 2:
                ms[name].append(e0.elapsed_time(e1))
    ws.sync(st)
    r = res.cpu().numpy()
    out = {"workload": "%d pairs of 2 x %d bases, subjects of %d bases (four target windows) cut from the configs[1] genomes; query step: "
                       "configs[1] table, %d species x 10 strains, %d reads x %d bases, emulate_ranks 2, max_cand 2" % (B, L, S, n_species, B, L),
           "reps": a.reps}
    for k, v in ms.items():
        out[k] = {"ms_per_call": float(np.median(v)), "ms_min": float(min(v)), "ms_max": float(max(v))}
    out["ms_per_1M_pairs"] = out["align"]["ms_per_call"] * (1 << 20) / B
    out["ratio_to_query_step"] = out["align"]["ms_per_call"] / out["query_step"]["ms_per_call"]
    out["answered"] = {"pairs_aligned": int((r[:, 1] > 0).sum()), "reverse_chosen": int(r[:, 2].sum()), "mean_score": float(r[:, 0].mean()),
                       "mean_aligned_length": float(r[:, 1].mean()), "pairs_beyond_capacity": int((r[:, 3] != 0).sum())}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
