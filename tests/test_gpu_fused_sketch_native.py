"""wave_sketch_two_windows (mcq_device.hpp: both windows of a 129..160-base read sketched in one pass) against wave_sketch per
window on the same bytes, on the GPU: every length, ambiguity codes and lower case on the window and k-mer boundaries, windows
with few k-mers, tandem repeats, reads back to back in an allocation of exactly their size -- with the threshold as shipped and
with thresholds that force the two retry paths (tests/native/fused_sketch.hip prints how many reads took each path)."""
import os
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_fused_sketch_against_the_sketch_per_window(tmp_path):
    exe = str(tmp_path / "fused_sketch")
    src = os.path.join(ROOT, "tests", "native", "fused_sketch.hip")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "metacache-mpi_amd", "csrc"),
                    "-I" + os.path.join(ROOT, "include"), src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAILED" not in r.stdout
