"""The --cost mi rows of the drop-in main's option table (host/main.cpp) without a GPU, beside
tests/test_main_perm_options_cpu.py: a bad value, an option without its cost and PatchMatch stereo are refused by the parser,
which returns before the device is probed -- exit status 2, the option's name on stderr, nothing on stdout.  A good command line
passes the parser: without a device it ends at the probe (exit status 1), with one it would run.  The conflicts with --ngpu and
--pipeline are decided behind the probe, and the options reach the context and the twins there: tests/test_gpu_main_mi.py."""
import subprocess

import pytest

from main_harness import binary  # noqa: F401  (a fixture)

M = ["--cost", "mi"]
BAD_VALUES = [M + ["--mi-iterations", "0"], M + ["--mi-iterations", "17"], M + ["--mi-iterations", "3x"], M + ["--mi-iterations"],
              M + ["--mi-init", "census"], M + ["--mi-init", "Random"], M + ["--mi-seed", "-1"], M + ["--mi-seed", "4294967296"],
              M + ["--mi-seed", "1.5"]]
WITHOUT_THE_COST = [["--mi-iterations", "2"], ["--mi-init", "reference"], ["--mi-seed", "3"],
                    ["--cost", "mi", "--cost", "census", "--mi-iterations", "2"]]
CONFLICTS = [M + ["--aggregation", "patchmatch"], ["--aggregation", "patchmatch", "--mi-init", "reference"] + M]


@pytest.mark.parametrize("args", BAD_VALUES + WITHOUT_THE_COST + CONFLICTS, ids=lambda a: "_".join(a).replace("-", ""))
def test_main_refuses_before_the_device_probe(binary, tmp_path, args):
    r = subprocess.run([binary] + args, cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, (r.returncode, r.stdout + r.stderr)
    assert "--mi-" in r.stderr or "--cost mi" in r.stderr, r.stderr
    assert r.stdout == ""


def test_an_unknown_cost_names_the_four(binary, tmp_path):
    r = subprocess.run([binary, "--cost", "nmi"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "`reference`, `census`, `adcensus` or `mi`" in r.stderr and r.stdout == ""


@pytest.mark.parametrize("args", [M, M + ["--mi-iterations", "1"], M + ["--mi-iterations", "16"], M + ["--mi-init", "random"],
                                  M + ["--mi-init", "reference", "--mi-seed", "4294967295"],
                                  M + ["--aggregation", "sgm"], M + ["--permeability", "32", "--guidance", "rgb"],
                                  ["--cost", "census"] + M + ["--mi-seed", "0"]],
                         ids=["alone", "one_table", "sixteen", "random", "reference_seed", "sgm", "perm_rgb", "last_cost_wins"])
def test_good_values_pass_the_parser(binary, tmp_path, args):
    """the parser prints nothing and does not return 2: the run gets as far as the device probe (and the missing input pair)"""
    r = subprocess.run([binary] + args, cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode != 2, r.stderr
    assert "needs" not in r.stderr and "unknown option" not in r.stderr and "cannot be combined" not in r.stderr
    assert r.stdout.startswith("Starting...")
