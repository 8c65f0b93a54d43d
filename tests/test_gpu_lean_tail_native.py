"""narrow_tail_lin (mcq_device.hpp: the lean first wave stage's tail without a sort, for at most 64 distinct keys and a window range
of at most 4) against dedup_finish -> sweep_targets_regs -> topk_lin_write on the same caller-made location lists, one wave per list,
on the GPU: D = 1, 2, 32, 33, 63, 64, multiplicities up to 200, ranges of 2, 3 and 4 windows that stop at a target's start, adjacent
words of different targets, look-ups that are displaced, miss behind foreign keys and wrap around the table, ties of every kind
under P = 2, 3, 4, 8 and M = 1, 2, 4, targets without a taxon (tests/native/lean_tail.hip prints how many lists took the tie
reduction and fails if none did)."""
import os
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_sort_free_tail_against_the_sorted_chain(tmp_path):
    exe = str(tmp_path / "lean_tail")
    src = os.path.join(ROOT, "tests", "native", "lean_tail.hip")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "metacache-mpi_amd", "csrc"),
                    "-I" + os.path.join(ROOT, "include"), src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAILED" not in r.stdout
    assert "took the tie reduction in all" in r.stdout
