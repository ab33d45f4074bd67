"""The command line of the drop-in main (host/main.cpp) without a GPU: a bad value, an option outside its mode, a missing
value and an unknown option are refused by the parser, which returns before the device is probed -- exit status 2, the
option's name on stderr, nothing on stdout."""
import subprocess

import pytest

from main_harness import binary  # noqa: F401  (a fixture)

BAD_VALUES = [["--wmf", "some"], ["--subpixel", "cubic"], ["--cost", "sad"], ["--adcensus-lambda", "30"],
              ["--adcensus-scale", "0"], ["--ad", "hsv"], ["--census-window", "4x3"], ["--census-th", "0"],
              ["--aggregation", "semi"], ["--cross-arms", "64,1"], ["--cross-tau", "6,20"], ["--cross-iterations", "5"],
              ["--sgm-p", "11,10"], ["--sgm-paths", "6"], ["--speckle", "5,-1"], ["--uniqueness", "100"],
              ["--guidance", "colour"]]
OUTSIDE_ITS_MODE = [["--census-th", "9"], ["--ad", "rgb"], ["--sgm-p", "5,40"], ["--cross-arms", "17,8"]]
CASES = BAD_VALUES + OUTSIDE_ITS_MODE + [["--pfm"], ["--no-such-option"]]


@pytest.mark.parametrize("args", CASES, ids=lambda a: "_".join(a).lstrip("-"))
def test_main_refuses_before_the_device_probe(binary, tmp_path, args):
    r = subprocess.run([binary] + args, cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, (r.returncode, r.stdout + r.stderr)
    assert args[0] in r.stderr, r.stderr
    assert r.stdout == ""
