"""The --permeability row of the drop-in main's option table (host/main.cpp) without a GPU, beside
tests/test_main_patchmatch_options_cpu.py: a bad value and an aggregation the filter does not run behind are refused by the
parser, which returns before the device is probed -- exit status 2, the option's name on stderr, nothing on stdout.  A good
command line passes the parser: without a device it ends at the probe (exit status 1), with one it would run.  The conflicts
with --ngpu and --pipeline are decided behind the probe: tests/test_gpu_main_perm.py."""
import subprocess

import pytest

from main_harness import binary  # noqa: F401  (a fixture)

P = ["--permeability"]
BAD_VALUES = [P + ["0"], P + ["0.0"], P + ["32x"], P + ["1,2"], P + ["1e999"], P + ["32", "--permeability", "0"]]
CONFLICTS = [P + ["--aggregation", a] for a in ("sgm", "cross", "scanline", "cross-scanline", "patchmatch")] + \
            [["--aggregation", "sgm"] + P + ["16"], P + ["--cross-scale"], ["--cross-scale", "2"] + P + ["8"]]


@pytest.mark.parametrize("args", BAD_VALUES + CONFLICTS, ids=lambda a: "_".join(a).replace("-", ""))
def test_main_refuses_before_the_device_probe(binary, tmp_path, args):
    r = subprocess.run([binary] + args, cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, (r.returncode, r.stdout + r.stderr)
    assert "--permeability" in r.stderr, r.stderr
    assert r.stdout == ""


@pytest.mark.parametrize("args", [P, P + ["32"], P + ["0.001"], P + ["1e6"], P + ["--guidance", "rgb", "--cost", "census"],
                                  P + ["--aggregation", "guided"]],
                         ids=["alone", "32", "0.001", "1e6", "rgb_census", "guided"])
def test_good_values_pass_the_parser(binary, tmp_path, args):
    """the parser prints nothing and does not return 2: the run gets as far as the device probe (and the missing input pair)"""
    r = subprocess.run([binary] + args, cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode != 2, r.stderr
    assert "needs" not in r.stderr and "unknown option" not in r.stderr and "cannot be combined" not in r.stderr
    assert r.stdout.startswith("Starting...")
