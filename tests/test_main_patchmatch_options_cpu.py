"""The PatchMatch rows of the drop-in main's option table (host/main.cpp) without a GPU, beside tests/test_main_options_cpu.py:
a bad value and a --pm-* option outside --aggregation patchmatch are refused by the parser, which returns before the device is
probed -- exit status 2, the option's name on stderr, nothing on stdout.  A good command line passes the parser: without a
device it ends at the probe (exit status 1), with one it would run.  The conflicts with other stages are decided behind the
probe: tests/test_gpu_main_patchmatch.py."""
import subprocess

import pytest

from main_harness import binary  # noqa: F401  (a fixture)

PM = ["--aggregation", "patchmatch"]
BAD_VALUES = [PM + ["--pm-radius", "18"], PM + ["--pm-radius", "-1"], PM + ["--pm-radius", "2.5"], PM + ["--pm-gamma", "0"],
              PM + ["--pm-gamma", "inf"], PM + ["--pm-gamma", "ten"], PM + ["--pm-iterations", "0"], PM + ["--pm-iterations", "17"],
              PM + ["--pm-slope", "-0.1"], PM + ["--pm-slope", "8.5"], PM + ["--pm-seed", "-1"], PM + ["--pm-seed", "4294967296"],
              PM + ["--pm-seed", "1x"]]
OUTSIDE_ITS_MODE = [["--pm-radius", "4"], ["--pm-gamma", "10"], ["--pm-iterations", "2"], ["--pm-slope", "1"], ["--pm-seed", "3"],
                    ["--aggregation", "sgm", "--pm-radius", "4"], PM + ["--aggregation", "guided", "--pm-seed", "3"]]
MISSING_VALUE = [PM + ["--pm-radius"], ["--aggregation", "patch-match"]]


@pytest.mark.parametrize("args", BAD_VALUES + OUTSIDE_ITS_MODE + MISSING_VALUE, ids=lambda a: "_".join(a).replace("-", ""))
def test_main_refuses_before_the_device_probe(binary, tmp_path, args):
    r = subprocess.run([binary] + args, cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, (r.returncode, r.stdout + r.stderr)
    named = [a for a in args if a.startswith("--pm-")] or ["--aggregation"]
    assert any(n in r.stderr for n in named), r.stderr
    assert r.stdout == ""


@pytest.mark.parametrize("args", [PM, PM + ["--pm-radius", "0"], PM + ["--pm-radius", "17", "--pm-gamma", "0.5", "--pm-iterations", "16",
                                            "--pm-slope", "8", "--pm-seed", "4294967295"], PM + ["--pm-slope", "0"]],
                         ids=["alone", "radius_0", "the_ends", "slope_0"])
def test_good_values_pass_the_parser(binary, tmp_path, args):
    """the parser prints nothing and does not return 2: the run gets as far as the device probe (and the missing input pair)"""
    r = subprocess.run([binary] + args, cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode != 2, r.stderr
    assert "needs" not in r.stderr and "unknown option" not in r.stderr
    assert r.stdout.startswith("Starting...")
