#!/usr/bin/env python3
"""SGPR-spill moves of the lean first wave stage, basic block by basic block (device ISA via hipcc -S, as scripts/isa_stats.py).
python3 scripts/lean_loop_spills.py [KERNEL_REGEX] [--src FILE.s | unit of csrc/] [--all]

For every basic block inside the per-read loop that holds a v_readlane_b32 / v_writelane_b32 it prints the block's label, its
instruction count, the lane moves, and of the restored SGPRs how many are READ in the block, how many are still live when the block
ends (not judged: a later block may read them) and how many are DEAD: overwritten before anything read them.  Blocks are named by
what they hold:
  loop-top      the block behind the loop header (the two sequence offsets)
  sketch        ds_bpermute_b32 (wave_sketch_two_windows / wave_sketch_b)
  table-clear   two ds_write_b128 and more (dedup_insert)
  insert        ds_cmpst_rtn_b32 (dedup_insert)
  result-write  global_store_dwordx4 (the candidates)
  ncand-write   global_store_dword with a scalar base (out.ncand[q])
  queue         global_atomic_* / global_store_dword with a vector address (hand-over to the later stages)
It then checks the three blocks section 23 of DESIGN.md is about: result-write, ncand-write and table-clear blocks restore only
registers they read (no DEAD restores, and no restores at all where the block's own instructions read none).  Exit status 1 if not.
The count is of text.  Which blocks a read executes is the dynamic count's business (rocprofv3 --pmc)."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
args = sys.argv[1:]
show_all = "--all" in args
if show_all:
    args.remove("--all")
src = os.path.join(ROOT, "metacache-mpi_amd", "csrc", "mcq_engine.hip")
if "--src" in args:
    i = args.index("--src"); src = args[i + 1]; del args[i:i + 2]
    if os.sep not in src and not os.path.exists(src):
        src = os.path.join(ROOT, "metacache-mpi_amd", "csrc", src)
pat = re.compile(args[0] if args else r"k_query_waveIjLi512ELb0ELb0ELb0ELi2ELi1ELb1ELb0ELb0ELb0E")
asm = src if src.endswith(".s") else "/tmp/lean_loop_spills_%d.s" % os.getpid()
if not src.endswith(".s"):
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", src, "-o", asm],
                   check=True, stderr=subprocess.DEVNULL)
lines = open(asm).read().split("\n")

SREG = re.compile(r"\bs(\d+)\b|\bs\[(\d+):(\d+)\]")


def sregs(text):
    out = set()
    for m in SREG.finditer(text):
        if m.group(1) is not None:
            out.add(int(m.group(1)))
        else:
            out.update(range(int(m.group(2)), int(m.group(3)) + 1))
    return out


def operands(ins):
    """(defined SGPRs, read SGPRs) of one instruction: the first operand is the destination, except for stores, compares into
    vcc / exec and branches; good enough for telling a restored register that is read from one that is overwritten"""
    parts = ins.split(None, 1)
    op, rest = parts[0], (parts[1] if len(parts) > 1 else "")
    ops = [o.strip() for o in rest.split(",")]
    if op.startswith(("global_store", "ds_write", "s_cmp", "s_bitcmp", "s_cbranch", "s_branch", "s_waitcnt", "s_nop", "v_cmpx", "global_atomic", "buffer_store")) \
            or (op.startswith("v_cmp") and op.endswith("_e32")):
        return set(), sregs(rest)
    return sregs(ops[0]) if ops else set(), sregs(",".join(ops[1:]))


def blocks_of(fn):
    cur = None
    out = []
    for no, l in fn:
        t = l.strip()
        m = re.match(r"^(\.LBB\d+_\d+):|^; (%bb\.\d+):", t)
        if m:
            cur = {"label": m.group(1) or m.group(2), "line": no, "ins": [], "depth": 1 if "in Loop" in t or "Loop Header" in t or "Parent Loop" in t else 0,
                   "header": "This Loop Header: Depth=1" in t}
            out.append(cur)
            continue
        if cur is None or not t or t[0] in ";." or t.endswith(":"):
            continue
        cur["ins"].append(t.split(";")[0].strip())
    return out


def tags_of(b, after_header):
    ops = [i.split()[0] for i in b["ins"]]
    t = []
    if after_header: t.append("loop-top")
    if "ds_bpermute_b32" in ops: t.append("sketch")
    if ops.count("ds_write_b128") >= 2: t.append("table-clear")
    if "ds_cmpst_rtn_b32" in ops: t.append("insert")
    if "global_store_dwordx4" in ops: t.append("result-write")
    for i in b["ins"]:
        if i.startswith("global_store_dword "):
            t.append("ncand-write" if re.search(r", s\[\d+:\d+\]", i) else "queue")
    if any(o.startswith("global_atomic") for o in ops) and "queue" not in t: t.append("queue")
    return t


def judge(b):
    """restores of the block: read / live at the block's end / dead"""
    read = live = dead = 0
    ins = b["ins"]
    for k, i in enumerate(ins):
        if not i.startswith("v_readlane_b32"):
            continue
        reg = next(iter(sregs(i.split(",")[0])))
        state = "live"
        for j in ins[k + 1:]:
            d, r = operands(j)
            if j.startswith("v_readlane_b32"):
                d, r = sregs(j.split(",")[0]), set()
            if j.startswith("v_writelane_b32"):
                d, r = set(), sregs(j)
            if reg in r: state = "read"; break
            if reg in d: state = "dead"; break
        read += state == "read"; live += state == "live"; dead += state == "dead"
    return read, live, dead


bad = 0
i = 0
while i < len(lines):
    m = re.match(r"^(_Z\w+):", lines[i])
    if not (m and pat.search(m.group(1))):
        i += 1
        continue
    j = i
    while not lines[j].startswith(".Lfunc_end"):
        j += 1
    print(m.group(1)[:100])
    tot_r = tot_w = loop_r = loop_w = 0
    prev_header = False
    print("  %-12s %6s %5s %5s %5s   %-16s %s" % ("block", "line", "ins", "rdln", "wrln", "read/live/dead", "holds"))
    for b in blocks_of(list(enumerate(lines[i + 1:j], i + 2))):
        r = sum(x.startswith("v_readlane_b32") for x in b["ins"]); w = sum(x.startswith("v_writelane_b32") for x in b["ins"])
        tot_r += r; tot_w += w
        tg = tags_of(b, b["header"])
        if b["depth"]:
            loop_r += r; loop_w += w
        named = [t for t in tg if t in ("result-write", "ncand-write", "table-clear")]
        rd, lv, dd = judge(b)
        if b["depth"] and (r or w or (show_all and tg) or named):
            print("  %-12s %6d %5d %5d %5d   %3d /%3d /%3d    %s" % (b["label"], b["line"], len(b["ins"]), r, w, rd, lv, dd, " ".join(tg)))
        if named and (dd or lv):
            bad += 1
            print("    ^ %s restores a register it does not read" % "/".join(named))
    print("  whole kernel: v_readlane %d  v_writelane %d;  inside the per-read loop: %d / %d" % (tot_r, tot_w, loop_r, loop_w))
    i = j
sys.exit(1 if bad else 0)
