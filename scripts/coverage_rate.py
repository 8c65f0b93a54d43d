#!/usr/bin/env python3
"""The price of mcq_coverage_add / mcq_coverage_read (the kernels behind -coverage and -cov-percentile) on bench.py's default table
(configs[1]: 50 species x 10 strains, 1 M reads of 150 bases, emulate_ranks 2, max_cand 2), n_slots 2, as scripts/target_hits_rate.py
measures mcq_target_hits: the slot targets come from the batch's own results at sequence level, mcq_target_hits answers them once, and
its outputs stay on the device as the input of every mcq_coverage_add call.  The add is measured twice -- on an empty bitmap (a reset
in front of every call, outside the events) and on a saturated one (the same batch again: loads only) -- beside mcq_target_hits and
the query step of the same session, and mcq_coverage_read (popcount kernel, copy, wait) by the host's clock.
Prints one JSON object: GPU milliseconds per call (median of --reps after 3 warm-up calls, events around each call, the kinds
alternating) and what the accumulator holds.
usage: python scripts/coverage_rate.py [--small] [--out profiles/coverage_rate.json]"""
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
    windows = table.tgt_windows()
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

    cov = eng.Coverage(windows, device=0)

    def add_saturated():
        cov.add(rng, cnt, B, n_slots, cap, stream=st)

    q_sequence()
    eng.target_slots(cands.data_ptr(), ncand.data_ptr(), B, 2, 1, tax2tgt.data_ptr(), n_targets, slots.data_ptr(), n_slots, stream=st)
    hits()
    torch.cuda.synchronize(dev)
    calls = {"query_species_keys": q_species, "target_hits": hits, "coverage_add_empty": add_saturated, "coverage_add_saturated": add_saturated}
    ms = {k: [] for k in calls}
    ms["coverage_read_host_ms"] = []
    for i in range(3 + a.reps):
        for name, fn in calls.items():
            if name == "coverage_add_empty":
                cov.reset(stream=st)                                              # (in front of the first event: the memsets are not timed)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= 3:
                ms[name].append(e0.elapsed_time(e1))
        t0 = time.perf_counter()
        rec, oor = cov.read(stream=st)
        if i >= 3:
            ms["coverage_read_host_ms"].append((time.perf_counter() - t0) * 1e3)
    ws_seq.sync(st)                                                               # (raises if a read was beyond the kernel's capacity)
    cov.reset(stream=st)
    add_saturated()
    rec, oor = cov.read(stream=st)
    r = rng.cpu().numpy().view(np.uint32)
    used = r[:, :, 0] != 0xFFFFFFFF
    out = {"workload": "configs[1] table, %d species x 10 strains, %d reads x %d bases, emulate_ranks 2, max_cand 2; n_slots %d, range_cap %d"
                       % (n_species, B, L, n_slots, cap),
           "reps": a.reps}
    for k, v in ms.items():
        out[k] = {"ms_per_call": float(np.median(v)), "ms_min": float(min(v)), "ms_max": float(max(v))}
    for k in ("coverage_add_empty", "coverage_add_saturated"):
        out[k]["ms_per_1M_reads"] = out[k]["ms_per_call"] * (1 << 20) / B
        out[k]["ratio_to_target_hits"] = out[k]["ms_per_call"] / out["target_hits"]["ms_per_call"]
        out[k]["ratio_to_query_step"] = out[k]["ms_per_call"] / out["query_species_keys"]["ms_per_call"]
    out["count_words_per_call"] = int(B * n_slots * cap)
    out["accumulator"] = {"targets": int(len(windows)), "windows": int(np.asarray(windows, np.uint64).sum()), "bitmap_words": int(len(cov.bitmap()[0]) - 2),
                          "windows_covered": int(rec["windows_covered"].sum()), "entries": int(rec["queries"].sum()), "hits": int(rec["hits"].sum()),
                          "out_of_range": int(oor), "slots_used": int(used.sum()), "slots_with_a_range": int((r[:, :, 3] > 0).sum()),
                          "hits_in_ranges": int(r[:, :, 1].sum()), "queries_beyond_capacity": int((status != 0).sum().item())}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
