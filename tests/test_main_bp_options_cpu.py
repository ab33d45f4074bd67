"""The --aggregation bp rows of the drop-in main's option table (host/main.cpp) without a GPU, beside
tests/test_main_perm_options_cpu.py: a bad value, a --bp-* option without the aggregation and --permeability behind it are
refused by the parser, which returns before the device is probed -- exit status 2, the option's name on stderr, nothing on
stdout.  A good command line passes the parser: without a device it ends at the probe (exit status 1), with one it would run.
The conflicts with --guidance rgb, --cross-scale, --ngpu and --pipeline and the label bound are decided behind the probe:
tests/test_gpu_main_bp.py."""
import subprocess

import pytest

from main_harness import binary  # noqa: F401  (a fixture)

A = ["--aggregation", "bp"]
BAD_VALUES = [(A + ["--bp-step", "-1"], "--bp-step"), (A + ["--bp-step", "4096"], "--bp-step"), (A + ["--bp-step", "2x"], "--bp-step"),
              (A + ["--bp-trunc", "-1"], "--bp-trunc"), (A + ["--bp-trunc", "4096"], "--bp-trunc"),
              (A + ["--bp-iterations", "65"], "--bp-iterations"), (A + ["--bp-iterations", "-1"], "--bp-iterations"),
              (A + ["--bp-levels", "0"], "--bp-levels"), (A + ["--bp-levels", "9"], "--bp-levels"),
              (A + ["--bp-scale", "0"], "--bp-scale"), (A + ["--bp-scale", "-2"], "--bp-scale"), (A + ["--bp-scale", "1e999"], "--bp-scale"),
              (A + ["--bp-scale", "1e-60"], "--bp-scale"), (A + ["--bp-scale", "nan"], "--bp-scale"), (A + ["--bp-scale"], "--bp-scale"),
              (["--aggregation", "belief"], "--aggregation")]
NEED_BP = [(["--bp-step", "20"], "--bp-step"), (["--bp-trunc", "60"], "--bp-trunc"), (["--bp-iterations", "5"], "--bp-iterations"),
           (["--bp-levels", "4"], "--bp-levels"), (["--bp-scale", "16"], "--bp-scale"),
           (["--aggregation", "sgm", "--bp-levels", "4"], "--bp-levels"), (A + ["--aggregation", "guided", "--bp-step", "3"], "--bp-step"),
           (A + ["--sgm-p", "10,120"], "--sgm-p")]
CONFLICTS = [(A + ["--permeability"], "--permeability"), (["--permeability", "16"] + A, "--permeability")]


@pytest.mark.parametrize("args,name", BAD_VALUES + NEED_BP + CONFLICTS, ids=lambda a: "_".join(a).replace("-", "") if isinstance(a, list) else None)
def test_main_refuses_before_the_device_probe(binary, tmp_path, args, name):
    r = subprocess.run([binary] + args, cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, (r.returncode, r.stdout + r.stderr)
    assert name in r.stderr, r.stderr
    assert r.stdout == ""


@pytest.mark.parametrize("args", [A, A + ["--bp-step", "0", "--bp-trunc", "0"], A + ["--bp-step", "4095", "--bp-trunc", "4095"],
                                  A + ["--bp-iterations", "0"], A + ["--bp-iterations", "64", "--bp-levels", "8"],
                                  A + ["--bp-levels", "1", "--bp-scale", "16"], A + ["--bp-scale", "0.25", "--cost", "census"],
                                  ["--bp-scale", "2"] + A, A + ["--cost", "adcensus", "--uniqueness", "5", "--subpixel", "parabola"]],
                         ids=["alone", "zero_penalties", "largest_penalties", "no_iterations", "most", "one_level_scale", "census",
                              "option_first", "later_stages"])
def test_good_values_pass_the_parser(binary, tmp_path, args):
    """the parser prints nothing and does not return 2: the run gets as far as the device probe (and the missing input pair)"""
    r = subprocess.run([binary] + args, cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode != 2, r.stderr
    assert "needs" not in r.stderr and "unknown option" not in r.stderr and "cannot be combined" not in r.stderr
    assert r.stdout.startswith("Starting...")
