"""The tree filter in the persistent context's rules, without a GPU: smx_ctx_set_tree plans exactly as smx_ctx_set_permeability
does under every combination of the other stages and on every entry -- the same verdict, the same plan, the same row of the
stage table -- its refusals name the tree filter and smx_ctx_set_tree, never the permeability filter, and the two setters
refuse each other.

tests/host_ctx_plan_tree_check.cpp is the stand-alone program (csrc/smx_ctx_plan.h and nothing of the library), built twice with
the BUILDS of test_host_twins_cpu.py; the sanitised build is the program itself, nothing preloaded.  That the modes the context
had before plan as before is tests/test_ctx_plan_cpu.py, tests/test_ctx_plan_mi_cpu.py and tests/test_ctx_plan_zncc_cpu.py,
unchanged.

Run anywhere:  python -m pytest tests -q -m "not gpu" -k ctx_plan_tree
"""
import os
import shutil
import subprocess

import pytest

from test_host_twins_cpu import BUILDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stereo_matching_cuda_amd", "csrc")
WHY = "the tree filter runs over the guided filter's volumes of one scale"


@pytest.mark.parametrize("build", list(BUILDS))
def test_the_tree_filter_plans_as_permeability_does_under_its_own_name(tmp_path, build):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "host_ctx_plan_tree_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + BUILDS[build] +
                          ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(ROOT, "tests", "host_ctx_plan_tree_check.cpp"),
                           "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and r.stderr == "", r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    head = dict(zip(lines[0].split()[::2], map(int, lines[0].split()[1::2])))
    assert head["points"] == 3 * (1 << 17) and head["differ"] == 0 and head["misnamed"] == 0 and head["stages"] == 15
    assert 0 < head["ran"] < head["points"] // 8
    assert lines[1] == ("smx_ctx_stereo_pair: semi-global matching (smx_ctx_set_aggregation) and the tree filter (smx_ctx_set_tree) "
                        "do not run together: " + WHY)
    assert lines[2] == ("smx_ctx_stereo_pair: cross-scale aggregation (smx_ctx_set_cross_scale) and the tree filter "
                        "(smx_ctx_set_tree) do not run together: " + WHY)
    assert lines[3] == "smx_ctx_stereo_pair_async: the tree filter is on (smx_ctx_set_tree): use smx_ctx_stereo_pair"
    assert lines[4] == "smx_ctx_stereo_pair_async: the permeability filter is on (smx_ctx_set_permeability): use smx_ctx_stereo_pair"
    assert lines[5] == "smx_ctx_stereo_pair: the tree filter (smx_ctx_set_tree) produces no mean images"
    assert lines[6] == "alone: rc 0 perm 1 agg 1 cost 0 walker 1; off: perm 0 agg 0"
    # the mutual refusal names both setters; a mode does not refuse itself, and nothing refuses with both off
    assert lines[7].startswith("smx_ctx_set_tree: ") and "smx_ctx_set_permeability" in lines[7]
    assert lines[8].startswith("smx_ctx_set_permeability: ") and "smx_ctx_set_tree" in lines[8]
    assert lines[9] == "- - - -"
