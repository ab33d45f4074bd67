"""The ZNCC cost in the persistent context's rules, without a GPU: SMX_COST_ZNCC plans exactly as SMX_COST_CENSUS
does under every combination of the other stages and on every entry -- the same verdict, the same plan, the same row of the
stage table -- and its refusals name the ZNCC cost and smx_ctx_set_zncc, never census.

tests/host_ctx_plan_zncc_check.cpp is the stand-alone program (csrc/smx_ctx_plan.h and nothing of the library), built twice with
the BUILDS of test_host_twins_cpu.py; the sanitised build is the program itself, nothing preloaded.  That the modes the context
had before plan as before is tests/test_ctx_plan_cpu.py and tests/test_ctx_plan_mi_cpu.py, unchanged.

Run anywhere:  python -m pytest tests -q -m "not gpu" -k ctx_plan_zncc
"""
import os
import shutil
import subprocess

import pytest

from test_host_twins_cpu import BUILDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stereo_matching_cuda_amd", "csrc")


@pytest.mark.parametrize("build", list(BUILDS))
def test_zncc_plans_as_census_does_under_its_own_name(tmp_path, build):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "host_ctx_plan_zncc_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + BUILDS[build] +
                          ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(ROOT, "tests", "host_ctx_plan_zncc_check.cpp"),
                           "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and r.stderr == "", r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    head = dict(zip(lines[0].split()[::2], map(int, lines[0].split()[1::2])))
    assert head["points"] == 3 * (1 << 16) and head["differ"] == 0 and head["misnamed"] == 0 and head["stages"] == 15
    assert 0 < head["ran"] < head["points"] // 8
    assert lines[1] == ("smx_ctx_stereo_pair: PatchMatch stereo (smx_ctx_set_patchmatch) and the ZNCC cost "
                        "(smx_ctx_set_zncc) do not run together: PatchMatch stereo keeps no cost volume, and its planes are "
                        "sub-pixel already")
    assert lines[2] == "smx_ctx_stereo_pair_async: the ZNCC cost is on (smx_ctx_set_zncc): use smx_ctx_stereo_pair"
    assert lines[3] == "smx_ctx_stereo_pair_async: the census cost is on (smx_ctx_set_cost): use smx_ctx_stereo_pair"
    assert lines[4] == "alone: rc 0 census 1 cost 0; reference: census 0"
