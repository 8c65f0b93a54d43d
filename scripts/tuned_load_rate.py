#!/usr/bin/env python3
"""What the query-time bucket rules cost in the streaming loader (run on the GPU box from the repo root).

The benchmark's 2 Gbp table (50 species x 10 strains, 2 reference ranks) is built on the GPU and written as the reference's
shard files, as scripts/stream_load_at_scale.py does.  Then, in a fresh process per library, the files are loaded through the
streaming route (host.RefDb(meta_only).stream -> engine.PartsBuilder -> Parts.database), three runs each

    without a rule,  with keep_first = 128,  with removal above 127,

and one batch of the benchmark's reads (2^20 x 150 bp) is queried against each handle: ms per step before and after tuning.
With --parent-lib PATH (a libmcq_hip.so of the parent commit: scripts/ab_libs.sh) the load without a rule is also measured
with that library on the same box, so that "nothing new runs there" can be read off: the new library's three runs against
the parent's own spread.  Writes --out (default profiles/tuned_load_rate.json) and prints it."""
import argparse
import ctypes as C
import importlib
import json
import os
import shutil
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, S = 128, 113
CHUNK = 1 << 22              # locations per chunk, as include/mcq_open.hpp streams them


def write_shards(a, eng, host, synth, torch, dev):
    """the table as P shard files under a.workdir (prefix db) and one batch of reads as reads.npy / reads_off.npy"""
    P = a.ranks
    gb, goff, species = synth.make_genomes(a.species, a.strains, 2_000_000, 6_000_000, 0.02, seed=3, device=dev)
    n_targets = goff.numel() - 1
    r, ro, _ = synth.sample_reads(gb, goff, a.batch, 150, 0.005, 0.001, seed=1000)
    np.save(os.path.join(a.workdir, "reads.npy"), r.cpu().numpy()); np.save(os.path.join(a.workdir, "reads_off.npy"), ro.cpu().numpy())
    table = eng.Table(gb.data_ptr(), goff.data_ptr(), n_targets, emulate_ranks=P, device=0)
    glen = np.diff(goff.cpu().numpy().astype(np.int64))
    sp = species.cpu().numpy().astype(np.int64)
    del gb, r, ro
    torch.cuda.empty_cache()
    nk, nl = table.n_keys, table.n_locs
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

    def dev_tensor(ptr, n, dt):
        t = torch.empty(n, dtype=dt, device=dev)
        assert hip.hipMemcpy(t.data_ptr(), ptr, t.numel() * t.element_size(), 3) == 0          # device to device
        return t
    keys = dev_tensor(table.keys_ptr, nk, torch.int32)
    off = dev_tensor(table.list_off_ptr, nk + 1, torch.int64)
    locs = dev_tensor(table.locs_ptr, nl, torch.int64)
    table.close()
    nwin = np.where(glen <= W, 1, (glen - W) // S + 1 + (((glen - W) // S + 1) * S < glen))
    key_of = torch.repeat_interleave(torch.arange(nk, device=dev, dtype=torch.int32), off[1:] - off[:-1])
    total_bytes, longest = 0, 0
    for rk in range(P):
        sel = ((locs >> 32) % P) == rk
        l_r, k_r = locs[sel], key_of[sel]
        del sel
        kk, cnt = torch.unique_consecutive(k_r, return_counts=True)
        longest = max(longest, int(cnt.max().item()))
        keys_r = keys[kk.long()].cpu().numpy().view(np.uint32)
        o = np.zeros(kk.numel() + 1, np.uint64); o[1:] = np.cumsum(cnt.cpu().numpy())
        locs_r = l_r.cpu().numpy().view(np.uint64)
        del l_r, k_r, kk, cnt
        taxa = [dict(id=-(t + 1), parent=1000 + int(sp[t]), rank=0, name="genome_%d strain" % t, file="genomes/all.fna", index=t + 1,
                     windows=int(nwin[t]) if t % P == rk else 0) for t in range(n_targets - 1, -1, -1)]
        taxa.append(dict(id=1, parent=1, rank=20, name="root", file="", index=0, windows=0))
        taxa.append(dict(id=2, parent=1, rank=19, name="Bacteria", file="", index=0, windows=0))
        for s_ in sorted(set(int(x) for x in sp)):
            taxa.append(dict(id=1000 + s_, parent=2, rank=4, name="Synthetica species%d" % s_, file="", index=0, windows=0))
        path = os.path.join(a.workdir, "db.db_%d" % rk)
        host.write_shard(path, dict(k=16, sketch_size=16, winlen=W, winstride=S, q_k=16, q_sketch_size=16, q_winlen=W, q_winstride=S,
                                    max_locs_per_feature=254), taxa, n_targets, keys_r, o, locs_r)
        total_bytes += os.path.getsize(path)
    del key_of, locs, keys, off
    torch.cuda.empty_cache()
    return dict(db_bp=int(glen.sum()), db_keys=int(nk), db_locations=int(nl), targets=int(n_targets), shard_bytes=int(total_bytes),
                longest_bucket=longest)


def measure(a):
    """one process, one library: the loads and the query steps; prints one JSON object"""
    import torch
    eng = importlib.import_module("metacache-mpi_amd.engine")
    host = importlib.import_module("metacache-mpi_amd.host")
    dev = torch.device("cuda", 0)
    P = a.ranks
    r = torch.from_numpy(np.load(os.path.join(a.workdir, "reads.npy"))).to(dev)
    ro = torch.from_numpy(np.load(os.path.join(a.workdir, "reads_off.npy"))).to(dev)
    n_reads = ro.numel() - 1
    rules = {"no_rule": None} if a.measure == "parent" else {"no_rule": None, "keep_first_128": (128, 0), "remove_above_127": (0, 127)}
    out = {}
    for name, rule in rules.items():
        loads, counts, n_locs, db = [], None, None, None
        for _ in range(a.runs):
            if db is not None:
                db.close()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rdb = host.RefDb(os.path.join(a.workdir, "db"), P, meta_only=True)
            i = rdb.info
            pb = eng.PartsBuilder(rdb.tgt_windows(), k=i.k, sketch_size=i.q_sketch_size, winlen=i.q_winlen, winstride=i.q_winstride,
                                  tgt_winstride=i.winstride, expected_locations=i.n_locs)
            if rule is not None:
                pb.set_bucket_limit(*rule)
            for rk in range(P):
                for f, t, w in rdb.stream(rk, CHUNK):
                    pb.add(f, t, w)
            if rule is not None:
                counts = pb.bucket_counts()
            parts = pb.finish()
            n_locs = parts.n_locs
            t2t = rdb.tgt2tax(4)
            db = parts.database(t2t.ctypes.data, n_shards=1, shard_id=0, device_ptrs=False)
            parts.close()
            torch.cuda.synchronize()
            loads.append(round(time.perf_counter() - t0, 3))
        ws = eng.Workspace(db, n_reads, r.numel())
        cands = torch.zeros((n_reads, 2, 4), dtype=torch.int32, device=dev); ncand = torch.zeros(n_reads, dtype=torch.int32, device=dev)
        ms = []
        for step in range(a.warmup + a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ws.query_device(r.data_ptr(), ro.data_ptr(), n_reads, False, cands.data_ptr(), ncand.data_ptr(), max_cand=2, emulate_ranks=P,
                            flags=eng.MCQ_QUIRK_SEQ_DROP)
            e1.record()
            ws.sync(); torch.cuda.synchronize()
            if step >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        ws.close(); db.close()
        out[name] = dict(load_s=loads, locations_kept=int(n_locs), query_ms_per_step=round(float(np.median(ms)), 3),
                         query_ms_min_max=[round(min(ms), 3), round(max(ms), 3)], classified=int((ncand > 0).sum().item()))
        if counts is not None:
            out[name].update(buckets_shrunk=counts[0], buckets_removed=counts[1])
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--species", type=int, default=50)
    ap.add_argument("--strains", type=int, default=10)
    ap.add_argument("--ranks", type=int, default=2)
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workdir", default="/tmp/mcq_tuned_load")
    ap.add_argument("--parent-lib", default=None, help="libmcq_hip.so of the parent commit: its load without a rule, same box")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tuned_load_rate.json"))
    ap.add_argument("--measure", default=None, choices=["this", "parent"], help="(internal) the measuring process")
    a = ap.parse_args()
    if a.measure:
        return measure(a)
    import torch
    pkg = importlib.import_module("metacache-mpi_amd")
    pkg.build_hip(); pkg.build_host()
    eng = importlib.import_module("metacache-mpi_amd.engine")
    host = importlib.import_module("metacache-mpi_amd.host")
    synth = importlib.import_module("metacache-mpi_amd.synth")
    shutil.rmtree(a.workdir, ignore_errors=True)
    os.makedirs(a.workdir)
    res = {"table": "%d species x %d strains" % (a.species, a.strains), "reference_ranks": a.ranks, "reads_per_step": a.batch,
           "chunk_locations": CHUNK}
    t0 = time.time()
    res.update(write_shards(a, eng, host, synth, torch, torch.device("cuda", 0)))
    res["shard_files_written_s"] = round(time.time() - t0, 1)
    torch.cuda.empty_cache()

    def child(which, env):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--measure", which, "--workdir", a.workdir, "--ranks", str(a.ranks),
                            "--runs", str(a.runs), "--steps", str(a.steps), "--warmup", str(a.warmup)], env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True, timeout=1200)
        line = [l for l in p.stdout.split("\n") if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            return {"error": (p.stderr or p.stdout)[-1500:]}
        return json.loads(line[0][len("RESULT "):])
    res["this_commit"] = child("this", dict(os.environ))
    if a.parent_lib:
        res["parent_commit"] = child("parent", dict(os.environ, MCQ_HIP_LIB=os.path.abspath(a.parent_lib)))
        mine, par = res["this_commit"].get("no_rule", {}).get("load_s"), res["parent_commit"].get("no_rule", {}).get("load_s")
        if mine and par:
            res["no_rule_load_within_parents_spread"] = bool(min(par) <= float(np.median(mine)) <= max(par))
            res["no_rule_load_median_s"] = {"this": float(np.median(mine)), "parent": float(np.median(par))}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))
    shutil.rmtree(a.workdir, ignore_errors=True)
    return 0 if "error" not in res["this_commit"] else 1


if __name__ == "__main__":
    sys.exit(main() or 0)
