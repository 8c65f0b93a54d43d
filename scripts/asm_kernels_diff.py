#!/usr/bin/env python3
"""Device assembly of one translation unit in two states (hipcc -S --cuda-device-only --offload-arch=gfx950), compared kernel by
kernel after renumbering the basic-block labels in their order of appearance inside each kernel.  Prints one line per unit:
kernels on each side, identical ones, and the names of those that differ or exist on one side only.
usage: python scripts/asm_kernels_diff.py A.s B.s [A2.s B2.s ...]"""
import re
import sys


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+|\w+):\s*(;.*)?$", line)
        if name is None and m and not line.startswith("."):
            name, body = m.group(1), []
            continue
        if name is not None:
            if line.startswith(".Lfunc_end"):
                out[name] = body
                name = None
                continue
            s = line.split(";")[0].strip()                   # (comments carry offsets and source names)
            if s and not s.startswith((".p2align", ".loc", ".file", ".cfi")):
                body.append(s)
    return out


def renumber(body):
    seen = {}

    def sub(m):
        return seen.setdefault(m.group(0), ".L%d" % len(seen))
    return [re.sub(r"\.L[A-Za-z_]*\d+(_\d+)?", sub, l) for l in body]


def main():
    args = sys.argv[1:]
    for a, b in zip(args[0::2], args[1::2]):
        ka, kb = kernels(a), kernels(b)
        same = [k for k in ka if k in kb and renumber(ka[k]) == renumber(kb[k])]
        diff = [k for k in ka if k in kb and k not in same]
        only_a, only_b = [k for k in ka if k not in kb], [k for k in kb if k not in ka]
        print("%s | %s: %d / %d functions, %d identical line for line, %d differ, %d / %d on one side only, %d lines compared"
              % (a, b, len(ka), len(kb), len(same), len(diff), len(only_a), len(only_b), sum(len(ka[k]) for k in same)))
        for k in diff + only_a + only_b:
            print("   differs or is missing:", k)


if __name__ == "__main__":
    main()
