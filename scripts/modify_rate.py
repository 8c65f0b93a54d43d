#!/usr/bin/env python3
"""Extending a table against building it again, on the genome set of bench.py's table (run on the GPU box from the repo root).

The 50 species x 10 strains of bench.py's generator (2 Gbp, seed 3, 500 genomes).  In one process, alternating, --runs times each after one round of
warm-up:
  scratch   mcq_build_table of all 500 genomes (sequences in device memory)
  extend    mcq_table_extend_*: the table of the first 495 genomes as the triples its --ranks shard files hold -- in device memory, handed
            over file by file in chunks of --chunk triples, as mcq_build_cli -modify hands over what mcq_shard_stream_next gives -- then
            the last 5 genomes through finish
Every time is a host clock around calls that end in a device synchronise (both entry points synchronise before they return).  The
phases are the lines MCQ_BUILD_TRACE=1 makes the library print on stderr, read back from a file the descriptor is pointed at during
the call (the line of the last phase, "emit", also holds the time of the three before it: the pipeline's phase clock is a copy).  Not
in the extension's time: reading the shard files and copying their triples to the device (the program's "old
locations" phase does both; the from-scratch build's counterpart is reading 2 Gbp of FASTA).  The two tables are compared once.
Writes profiles/modify_rate.json, or the file --out names.
"""
import argparse
import importlib
import json
import os
import re
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class Stderr:
    """file descriptor 2 pointed at a file for the time of a call: the library's phase lines"""

    def __enter__(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile()
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2); os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode("latin-1")
        self.tmp.close()

    def phases(self):
        out = {}
        for m in re.finditer(r"^\[mcq_build\] (.+?)\s+([0-9.]+) s$", self.text, flags=re.M):
            out[m.group(1).strip()] = round(out.get(m.group(1).strip(), 0.0) + float(m.group(2)), 3)
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--species", type=int, default=50)
    ap.add_argument("--strains", type=int, default=10)
    ap.add_argument("--genome-min", type=int, default=3_000_000)
    ap.add_argument("--genome-max", type=int, default=5_000_000)
    ap.add_argument("--divergence", type=float, default=0.02)
    ap.add_argument("--new", type=int, default=5, help="genomes the extension adds (the last ones)")
    ap.add_argument("--ranks", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=1 << 22)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "modify_rate.json"))
    a = ap.parse_args()

    import torch
    os.environ["MCQ_BUILD_TRACE"] = "1"
    pkg = importlib.import_module("metacache-mpi_amd")
    pkg.build_hip()
    eng = importlib.import_module("metacache-mpi_amd.engine")
    synth = importlib.import_module("metacache-mpi_amd.synth")
    dev = torch.device("cuda", 0)
    P = a.ranks
    gb, goff, _ = synth.make_genomes(a.species, a.strains, a.genome_min, a.genome_max, a.divergence, seed=3, device=dev)
    n_all = goff.numel() - 1
    n_old = n_all - a.new
    res = {"table": "%d species x %d strains" % (a.species, a.strains), "targets": int(n_all), "db_bp": int(goff[-1]), "ranks": P,
           "old_targets": int(n_old), "new_targets": a.new, "new_bp": int(goff[-1] - goff[n_old]), "chunk_triples": a.chunk,
           "device": torch.cuda.get_device_name(0), "kernel_source_digest": pkg.source_digest()}

    # the old database: the table of the first n_old genomes as the triples of its P files, in device memory
    with Stderr():
        old = eng.Table(gb.data_ptr(), goff.data_ptr(), n_old, emulate_ranks=P, device=0)
    keys, loff, locs, win_off = old.to_host()
    old.close()
    res.update(old_keys=len(keys), old_locations=len(locs))
    old_windows = np.diff(win_off.astype(np.int64)).astype(np.uint32)
    feat = np.repeat(keys, np.diff(loff.astype(np.int64)))
    tgt, win = (locs >> np.uint64(32)).astype(np.uint32), (locs & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    del keys, loff, locs
    files = []
    for r in range(P):
        m = tgt % P == r
        files.append([torch.from_numpy(x[m].view(np.int32)).to(dev) for x in (feat, tgt, win)])
    n_old_locs = len(feat)
    del feat, tgt, win
    new_off = (goff[n_old:] - goff[n_old]).contiguous()
    new_bases = gb[int(goff[n_old]):]

    def scratch():
        torch.cuda.synchronize()
        with Stderr() as err:
            t0 = time.time()
            t = eng.Table(gb.data_ptr(), goff.data_ptr(), n_all, emulate_ranks=P, device=0)
            dt = time.time() - t0
        return t, dt, err.phases()

    def extend():
        torch.cuda.synchronize()
        with Stderr() as err:
            t0 = time.time()
            x = eng.TableExtend(old_windows, n_ranks=P, expected_old_locations=n_old_locs, device=0)
            for f, t_, w in files:
                for i in range(0, len(f), a.chunk):
                    n = min(a.chunk, len(f) - i)
                    x.add(f.data_ptr() + 4 * i, t_.data_ptr() + 4 * i, w.data_ptr() + 4 * i, n=n)
            t1 = time.time()
            t = x.finish(new_bases.data_ptr(), new_off.data_ptr(), a.new)
            t2 = time.time()
        return t, t2 - t0, t1 - t0, t2 - t1, err.phases()

    runs_s, runs_x, same = [], [], None
    for i in range(a.runs + 1):              # (the first round is the warm-up of both: code objects, the sort's first use)
        ts, dt, ph = scratch()
        runs_s.append({"wall_s": round(dt, 3), "phases_s": ph})
        tx, dt, d_add, d_fin, ph = extend()
        runs_x.append({"wall_s": round(dt, 3), "add_s": round(d_add, 3), "finish_s": round(d_fin, 3), "phases_s": ph})
        if same is None:
            a_, b_ = ts.to_host(), tx.to_host()
            same = all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a_, b_))
            res.update(db_keys=ts.n_keys, db_locations=ts.n_locs)
            del a_, b_
        ts.close(); tx.close()
    res["warm_up_round"] = {"from_scratch": runs_s.pop(0), "extension": runs_x.pop(0)}
    res["from_scratch"] = {"runs": runs_s, "wall_median_s": round(statistics.median(r["wall_s"] for r in runs_s), 3),
                           "wall_min_s": min(r["wall_s"] for r in runs_s), "wall_max_s": max(r["wall_s"] for r in runs_s)}
    res["extension"] = {"runs": runs_x, "wall_median_s": round(statistics.median(r["wall_s"] for r in runs_x), 3),
                        "wall_min_s": min(r["wall_s"] for r in runs_x), "wall_max_s": max(r["wall_s"] for r in runs_x),
                        "not_in_the_time": "reading the shard files and copying their triples to the device"}
    res["identical_tables"] = bool(same)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))
    if not same:
        sys.exit("the extended table differs from the one built from scratch")


if __name__ == "__main__":
    main()
