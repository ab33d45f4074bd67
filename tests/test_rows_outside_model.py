"""The comb walker's data flow with rows outside the image reduced to their column sums, on the CPU: tools/v5_model.cpp (comb
length 9, the shipped one) against the oracle, bit for bit, at the heights and widths of tests/test_gpu_rows_outside.py.  No
GPU: one g++ compile of the model, one run."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEIGHTS = list(range(21, 31)) + [1, 2, 9, 10, 11, 19, 20]
WIDTHS = (40, 200)


def test_model_with_outside_rows_equals_the_oracle(orc, tmp_path):
    exe = str(tmp_path / "v5_model")
    odir = os.path.join(ROOT, "oracle", "_build")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-DMODEL_L=9", os.path.join(ROOT, "tools", "v5_model.cpp"),
                           "-o", exe, "-L" + odir, "-lsmx_oracle", "-Wl,-rpath," + odir])
    shapes = [(w, h) for w in WIDTHS for h in HEIGHTS]
    p = subprocess.run([exe] + [str(v) for s in shapes for v in s], capture_output=True, text=True)
    lines = [l for l in p.stdout.split("\n") if l.strip()]
    assert p.returncode == 0 and len(lines) == len(shapes) and all("bit-exact" in l for l in lines), p.stdout + p.stderr
    # two strips at width 200, one at 40
    assert sum("K=2" in l for l in lines) == len(HEIGHTS) and sum("K=1" in l for l in lines) == len(HEIGHTS)
