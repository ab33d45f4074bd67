"""The CPU twins of the opt-in stages (host/cpu_twins.cpp: sgm_aggregateOnCPU, speckle_filterOnCPU, weighted_medianOnCPU)
against their independent numpy references (tests/sgm_ref.py, speckle_ref.py, wmf_ref.py), bit for bit, without a GPU.

The twins are what `smx_main --host-compare` trusts, so they are held to the references here, at the edges of the
contracts of include/smx.h, and once more under -fsanitize=address,undefined.  tests/host_twins_check.cpp is the
stand-alone program that runs them (no libsmx_hip.so, nothing loaded into python): it reads the cases this module writes
as raw files and writes the twins' outputs beside them; every comparison is made here.  The twins of the reference's own
stages have their sanitizer leg in tests/test_host_mirror.py (tests/host_sanitize_check.cpp); the main path that calls
sgm_aggregateOnCPU runs in tests/test_gpu_main_sgm.py.

Run anywhere:  python -m pytest tests -q -m "not gpu" -k host_twins
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import sgm_ref
import speckle_ref
import wmf_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "stereo_matching_cuda_amd", "host")
F32 = np.float32

BUILDS = {
    "plain": ["-O2"],
    # the flags of test_host_mirror.py::test_host_layer_and_oracle_under_sanitizers
    "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fsanitize=float-cast-overflow", "-fno-sanitize-recover=all",
                  "-fno-omit-frame-pointer"],
}


def _eq(a, b, name=""):
    """Bit for bit; two NaNs are equal whatever their payload or sign (as _eq of tests/test_gpu_sgm.py)."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (name, a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype == np.float32:
        both_nan = np.isnan(a) & np.isnan(b)
        a, b = a.view(np.uint32), b.view(np.uint32)
        a = np.where(both_nan, 0, a)
        b = np.where(both_nan, 0, b)
    bad = np.flatnonzero(a.ravel() != b.ravel())
    assert bad.size == 0, f"{name}: {bad.size} of {a.size} elements differ, first at {bad[:5]}"


def _bits(v):
    return "%08X" % int(np.array(v, F32).view(np.uint32))


# ---------------------------------------------------------------------------------------------
# the cases: {"line": the line of cases.txt, "stem", "inputs": {suffix: array}, "want": {suffix: array}}
# ---------------------------------------------------------------------------------------------
SGM_SHAPES = [(1, 1, 1), (1, 7, 2), (7, 1, 3), (5, 40, 9), (40, 5, 9), (33, 6, 65)]        # w, h, D
SGM_PENALTIES = [(10, 120), (0, 0), (7, 7), (4095, 4095)]


def _sgm_case(stem, cost, dmin, p1=10, p2=120, paths=8, agg=True, best=True, disp=True):
    D, h, w = cost.shape
    r = sgm_ref.outputs(cost, p1, p2, paths)
    want = {}
    if agg:
        want["agg.f32"] = r["agg"]
    if best:
        want["best.f32"] = r["best"]
    if disp:
        want["disp.f32"] = (dmin + r["z"]).astype(F32)
    line = f"sgm {stem} {w} {h} {D} {dmin} {p1} {p2} {paths} {int(agg)} {int(best)} {int(disp)}"
    return {"line": line, "stem": stem, "inputs": {"cost.f32": np.ascontiguousarray(cost, F32)}, "want": want, "ref": r}


def special_volume():
    """The volume of test_gpu_sgm.py::test_special_values_go_through_the_clamp."""
    w, h, D = 21, 5, 10
    specials = np.array([-1, -0.0, 0.0, 0.5, 254.999, 255, 255.5, 300, np.nan, np.inf, -np.inf, 1e30, -1e30, 1e-40], F32)
    rng = np.random.default_rng(9)
    cost = specials[rng.integers(0, specials.size, (D, h, w))]
    cost[0, 0, :2] = np.array([0xFFC00001, 0x7F800001], np.uint32).view(F32)         # a negative NaN, a signalling one
    assert set(np.unique(specials[~np.isnan(specials)]).tolist()) <= set(np.unique(cost[~np.isnan(cost)]).tolist())
    assert np.isnan(cost).sum() > 2
    return cost


def tie_volumes():
    """(a constant volume, one with exactly two equal minima per pixel, the larger of the two slices)"""
    w, h, D = 37, 6, 67
    const = np.full((D, h, w), 23, F32)
    rng = np.random.default_rng(5)
    two = rng.integers(10, 200, (D, h, w)).astype(F32)
    za = rng.integers(0, D, (h, w))
    zb = (za + rng.integers(1, D, (h, w))) % D
    np.put_along_axis(two, za[None], 3, axis=0)
    np.put_along_axis(two, zb[None], 3, axis=0)
    return const, two, np.maximum(za, zb)


def sgm_cases():
    out = []
    k = 0
    for w, h, D in SGM_SHAPES:
        for paths in (4, 8):
            for hi in (62, 255):
                cost = np.random.default_rng(w * 1000 + D + hi + paths).integers(0, hi + 1, (D, h, w)).astype(F32)
                for p1, p2 in SGM_PENALTIES:
                    dmin = (-(D - 1), 0, 5, -300)[k % 4]           # negative, zero, positive, far below zero
                    k += 1
                    out.append(_sgm_case(f"sgm_{w}x{h}x{D}_c{hi}_p{p1}_{p2}_r{paths}", cost, dmin, p1, p2, paths))
    sp = special_volume()
    for paths in (4, 8):
        out.append(_sgm_case(f"sgm_special_r{paths}", sp, -9, paths=paths))
        out.append(_sgm_case(f"sgm_special_flipped_r{paths}", sp[:, ::-1].copy(), 0, paths=paths))
    const, two, later = tie_volumes()
    D = const.shape[0]
    for paths in (4, 8):
        c = _sgm_case(f"sgm_tie_const_r{paths}", const, 0, 10, 120, paths)
        assert (c["want"]["disp.f32"] == D - 1).all() and (c["want"]["best.f32"] == paths * 23).all()     # the LAST slice
        out.append(c)
        out.append(_sgm_case(f"sgm_tie_const_p0_r{paths}", const, -(D - 1), 0, 0, paths))
        c = _sgm_case(f"sgm_tie_two_r{paths}", two, 0, 0, 0, paths)
        assert (c["want"]["disp.f32"] == later).all() and (c["want"]["best.f32"] == paths * 3).all()      # the later minimum
        out.append(c)
    cost = np.random.default_rng(77).integers(0, 63, (9, 11, 23)).astype(F32)
    for name, kw in (("agg", {"agg": False}), ("best", {"best": False}), ("disp", {"disp": False}),
                     ("agg_best", {"agg": False, "best": False}), ("all", {"agg": False, "best": False, "disp": False})):
        out.append(_sgm_case(f"sgm_null_{name}", cost, -8, 7, 50, 4, **kw))
    return out


def _speckle_case(stem, d, vmin, new_val, max_size, max_diff):
    h, w = d.shape
    want = speckle_ref.speckle_filter(d, vmin, new_val, max_size, max_diff)
    line = f"speckle {stem} {w} {h} {_bits(vmin)} {_bits(new_val)} {max_size} {_bits(max_diff)}"
    return {"line": line, "stem": stem, "inputs": {"disp.f32": np.ascontiguousarray(d, F32)}, "want": {"out.f32": want}}


def messy_speckle_map(rng, h, w, vmin, size_d):
    """Labels vmin .. vmin + size_d - 1 with every value the contract singles out mixed in."""
    d = (vmin + rng.integers(0, size_d, size=(h, w))).astype(F32)
    m = rng.random((h, w))
    specials = [np.nan, np.inf, -np.inf, -0.0, 2.0 ** 31, -2.0 ** 31, 3e38, -3e38, vmin - 100,
                vmin - 0.5, vmin - 0.999,               # just below vmin: the truncation toward zero reaches it (vmin <= 0)
                vmin - 1, vmin - 1.25, vmin + 0.25, vmin + 1.75]
    for i, v in enumerate(specials):
        d[(m >= 0.02 * i) & (m < 0.02 * (i + 1))] = v
    return d, specials


def speckle_cases():
    out = []
    for h, w in [(1, 1), (1, 40), (40, 1), (33, 29)]:
        d = np.random.default_rng(h * 1000 + w).integers(0, 4, size=(h, w)).astype(F32)
        verdicts = set()
        for max_size in sorted({0, 1, 7, w * h}):
            c = _speckle_case(f"spk_{h}x{w}_s{max_size}", d, 0, -100, max_size, 0)
            verdicts |= set(np.unique(c["want"]["out.f32"] == -100).tolist())
            if max_size == 0:
                _eq(c["want"]["out.f32"], d, "max_size 0 copies the map")
            out.append(c)
        assert verdicts == {False, True}
        out.append(_speckle_case(f"spk_{h}x{w}_s7_d1", d, 0, -100, 7, 1))
    for name, (d, cases) in speckle_ref.structured(21, 24).items():
        for max_diff, largest in cases:
            _, size = speckle_ref.components(d, 0, max_diff)
            big = int(size.max())
            assert largest is None or big == largest, (name, max_diff)
            for max_size in (big - 1, big):       # one below a component's size: it stays; equal to it: it goes
                c = _speckle_case(f"spk_{name.replace(' ', '_')}_d{max_diff}_s{max_size}", d, 0, -100, max_size, max_diff)
                assert bool(np.all(c["want"]["out.f32"] == -100)) == (max_size == big), (name, max_diff, max_size)
                out.append(c)
    rng = np.random.default_rng(23)
    vmin = -10
    d, specials = messy_speckle_map(rng, 35, 41, vmin, 6)
    present = d[~np.isnan(d)]
    assert all((present == F32(v)).any() for v in specials if v == v) and np.isnan(d).any()
    counting = speckle_ref.counts(d, vmin)
    assert counting[d == F32(vmin - 0.5)].all() and counting[d == F32(vmin - 0.999)].all()     # (int)-10.5 = -10 >= vmin
    assert not counting[d == F32(vmin - 1)].any() and not counting[d == F32(vmin - 100)].any()
    assert counting[d == F32(2.0 ** 31)].all() and not counting[d == F32(-2.0 ** 31)].any()
    for max_size, max_diff in ((5, 1.0), (40, 0.0), (3, 0.25), (0, 1.0), (35 * 41, 3.4e38)):
        out.append(_speckle_case(f"spk_messy_s{max_size}_d{max_diff}", d, vmin, vmin - 100, max_size, max_diff))
    frac = (rng.integers(0, 8, size=(35, 41)) * 0.25).astype(F32)          # a sub-pixel map
    for max_size, max_diff in ((6, 0.5), (60, 0.5), (6, 0.0), (6, 0.3)):
        out.append(_speckle_case(f"spk_frac_s{max_size}_d{max_diff}", frac, 0, -100, max_size, max_diff))
    return out


def _wmf_case(stem, guide, disp, dmin, size_d, select=None, radius=9, sigma_s=9.0, sigma_c=25.5):
    h, w = disp.shape
    ws, wc = wmf_ref.weight_tables(radius, sigma_s, sigma_c)       # the formula of include/smx.h in numpy
    want = wmf_ref.weighted_median(guide, disp, dmin, size_d, select, radius, ws, wc)
    line = f"wmf {stem} {w} {h} {dmin} {size_d} {radius} {sigma_s!r} {sigma_c!r} {int(select is not None)}"
    inputs = {"guide.u8": np.ascontiguousarray(guide, np.uint8), "disp.f32": np.ascontiguousarray(disp, F32)}
    if select is not None:
        inputs["select.f32"] = np.ascontiguousarray(select, F32)
    return {"line": line, "stem": stem, "inputs": inputs, "want": {"out.f32": want}, "tables": (ws, wc)}


def messy_wmf_map(rng, h, w, dmin, size_d):
    """Labels in range with NaN, +-inf, the LR marker, fractions, labels out of range and -0.0 mixed in."""
    d = (dmin + rng.integers(0, size_d, size=(h, w))).astype(F32)
    m = rng.random((h, w))
    d[m < 0.04] = np.nan
    d[(m >= 0.04) & (m < 0.06)] = np.inf
    d[(m >= 0.06) & (m < 0.08)] = -np.inf
    d[(m >= 0.08) & (m < 0.12)] = dmin - 100
    d[(m >= 0.12) & (m < 0.15)] += 0.25
    d[(m >= 0.15) & (m < 0.17)] = dmin + size_d
    d[(m >= 0.17) & (m < 0.19)] = -0.0
    d[(m >= 0.19) & (m < 0.20)] = dmin - 1
    d[(m >= 0.20) & (m < 0.21)] = 3e9
    return d


def occlusion_like(rng, h, w, dmin):
    """A select map: the LR marker on about a third of the pixels, labels elsewhere, and NaN / +-inf (select nothing)."""
    s = np.where(rng.random((h, w)) < 0.35, F32(dmin - 100), F32(dmin + 2)).astype(F32)
    m = rng.random((h, w))
    s[m < 0.05] = np.nan
    s[(m >= 0.05) & (m < 0.08)] = np.inf
    s[(m >= 0.08) & (m < 0.11)] = -np.inf
    s[(m >= 0.11) & (m < 0.14)] = dmin - 0.5           # truncates to dmin: not selected
    if s.size >= 8:                                    # every kind at least once, whatever the seed
        at = rng.permutation(s.size)[:6]
        s.ravel()[at] = [np.nan, np.inf, -np.inf, dmin - 0.5, dmin - 100, dmin + 2]
    return s


def wmf_cases():
    out = []
    # exact ties: a flat guide and a flat spatial table give every sample the same weight, and every window (the whole
    # image) holds as many samples of the one label as of the other: 2 * cum == total at the SMALLER label, which wins
    tie = np.where(np.arange(6)[None, :] < 3, F32(-4), F32(9)).repeat(4, 0)
    c = _wmf_case("wmf_ties", np.full((4, 6), 77, np.uint8), tie, -10, 24, None, 15, 1e6, 25.5)
    assert (c["tables"][0] == 1023).all() and (c["want"]["out.f32"] == -4).all()
    out.append(c)
    for h, w, radius in [(1, 1, 9), (1, 60, 9), (60, 1, 9), (3, 5, 15), (37, 40, 9), (9, 50, 4), (9, 50, 1)]:
        rng = np.random.default_rng(h * 7 + w + radius)
        g = rng.integers(0, 256, size=(h, w), dtype=np.uint8)
        d = messy_wmf_map(rng, h, w, -10, 24)
        sel = occlusion_like(rng, h, w, -10)
        if h * w >= 8:
            assert np.isnan(sel).any() and np.isinf(sel).any()
            picked = wmf_ref.selected(sel, -10, sel.shape)
            assert picked.any() and not picked.all() and not picked[~np.isfinite(sel)].any()
        out.append(_wmf_case(f"wmf_{h}x{w}_r{radius}_all", g, d, -10, 24, None, radius))
        out.append(_wmf_case(f"wmf_{h}x{w}_r{radius}_sel", g, d, -10, 24, sel, radius))
    # a second pair of sigmas, so small that most weights round to 0
    rng = np.random.default_rng(101)
    g = rng.integers(0, 256, size=(19, 33), dtype=np.uint8)
    d = messy_wmf_map(rng, 19, 33, -10, 24)
    for radius in (9, 1):
        c = _wmf_case(f"wmf_small_sigmas_r{radius}", g, d, -10, 24, None, radius, 1.0, 2.0)
        ws, wc = c["tables"]
        assert ws[0] == wc[0] == 1023 and (wc == 0).sum() > 240 and (radius == 1 or (ws == 0).sum() > ws.size // 2)
        out.append(c)
    out.append(_wmf_case("wmf_small_sigmas_sel", g, d, -10, 24, occlusion_like(rng, 19, 33, -10), 4, 0.75, 1.5))
    # windows without one counting sample (total 0): the output is disp[p], NaN included
    d0 = messy_wmf_map(rng, 19, 33, -10, 24)
    junk = np.array([np.nan, 0.5, 1e9, -np.inf, -110, 14, -11], F32)
    d0[2:17, 3:20] = junk[rng.integers(0, junk.size, (15, 17))]
    assert (wmf_ref.labels(d0, -10, 24)[2:17, 3:20] < 0).all()
    for radius in (4, 1):
        c = _wmf_case(f"wmf_total0_r{radius}", g, d0, -10, 24, None, radius)
        inner = (slice(2 + radius, 17 - radius), slice(3 + radius, 20 - radius))
        _eq(c["want"]["out.f32"][inner], d0[inner], "a window of total 0 keeps disp[p]")
        assert np.isnan(d0[inner]).any() and np.any(c["want"]["out.f32"] != d0)
        out.append(c)
    # the label ranges
    for dmin, size_d in [(0, 1), (-7, 1), (-15, 16), (5, 17), (2 ** 31 - 5, 4)]:
        rng = np.random.default_rng(size_d + 7)
        h, w = 12, 31
        g = rng.integers(0, 256, size=(h, w), dtype=np.uint8)
        if dmin < 2 ** 30:
            d = messy_wmf_map(rng, h, w, dmin, size_d)
            if size_d == 1:                       # a second value beside the one label, so that the map is not constant
                d[rng.random((h, w)) < 0.2] = dmin + 1
        else:                                     # no f32 lies in [2^31 - 5, 2^31 - 1): nothing counts, the map is copied
            vals = np.array([2.0 ** 31 - 128, 2.0 ** 31, 2.0 ** 31 + 256, -2.0 ** 31, 0, 3, np.nan, np.inf], F32)
            d = vals[rng.integers(0, vals.size, (h, w))]
        sel = occlusion_like(rng, h, w, dmin) if dmin < 2 ** 30 else np.where(rng.random((h, w)) < 0.5, F32(0), F32(2.0 ** 31))
        for name, s in (("all", None), ("sel", sel)):
            c = _wmf_case(f"wmf_range_{dmin}_{size_d}_{name}", g, d, dmin, size_d, s, 4)
            if dmin >= 2 ** 30:
                _eq(c["want"]["out.f32"], d, "nothing counts")
            out.append(c)
    return out


_CASES = {}


def cases():
    """All cases with the references' outputs, computed once and never changed."""
    if not _CASES:
        all_ = sgm_cases() + speckle_cases() + wmf_cases()
        assert len({c["stem"] for c in all_}) == len(all_), "stems must be unique"
        for c in all_:
            for a in list(c["inputs"].values()) + list(c["want"].values()):
                a.setflags(write=False)
        _CASES["all"] = all_
    return _CASES["all"]


# ---------------------------------------------------------------------------------------------
# the table reaches what it says
# ---------------------------------------------------------------------------------------------
def test_the_case_table_covers_every_stage_and_edge():
    cs = cases()
    stages = [c["line"].split()[0] for c in cs]
    assert stages.count("sgm") == len(SGM_SHAPES) * 2 * 2 * len(SGM_PENALTIES) + 4 + 6 + 5
    assert stages.count("speckle") and stages.count("wmf") and set(stages) == {"sgm", "speckle", "wmf"}
    sgm = [c["line"].split() for c in cs if c["line"].startswith("sgm ")]
    assert {(int(f[2]), int(f[3]), int(f[4])) for f in sgm} >= set(SGM_SHAPES)
    assert {int(f[8]) for f in sgm} == {4, 8} and {(int(f[6]), int(f[7])) for f in sgm} >= set(SGM_PENALTIES)
    dmins = {int(f[5]) for f in sgm}
    assert min(dmins) < 0 and 0 in dmins and max(dmins) > 0
    for k in (9, 10, 11):                          # each optional output is NULL in some case and requested in most
        assert {f[k] for f in sgm} == {"0", "1"}
    wmf = [c["line"].split() for c in cs if c["line"].startswith("wmf ")]
    assert {(int(f[4]), int(f[5])) for f in wmf} >= {(0, 1), (-7, 1), (-15, 16), (5, 17), (2 ** 31 - 5, 4)}
    assert {int(f[6]) for f in wmf} >= {1, 4, 9, 15} and {f[9] for f in wmf} == {"0", "1"}
    assert {(int(f[3]), int(f[2])) for f in wmf} >= {(1, 1), (1, 60), (60, 1), (3, 5), (37, 40), (9, 50)}
    spk = [c["line"].split() for c in cs if c["line"].startswith("speckle ")]
    assert {(int(f[3]), int(f[2])) for f in spk} >= {(1, 1), (1, 40), (40, 1), (33, 29)}
    assert "0" in {f[6] for f in spk} and _bits(0.0) in {f[7] for f in spk} and _bits(0.25) in {f[7] for f in spk}


# ---------------------------------------------------------------------------------------------
# the two builds
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", list(BUILDS))
def test_host_twins_equal_their_references(tmp_path, build):
    """Every case of cases() through tests/host_twins_check.cpp: exit status 0, a clean stderr (no sanitizer report in the
    sanitized build, which is the program itself, nothing preloaded), and every output equal to the reference's bits."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    cs = cases()
    exe = str(tmp_path / "host_twins_check")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off"] + BUILDS[build] +
                          ["-I" + os.path.join(ROOT, "include"), "-I" + HOST, os.path.join(ROOT, "tests", "host_twins_check.cpp"),
                           os.path.join(HOST, "cpu_twins.cpp"), "-o", exe])
    work = tmp_path / "cases"
    work.mkdir()
    (work / "cases.txt").write_text("\n".join(c["line"] for c in cs) + "\n")
    for c in cs:
        for suffix, a in c["inputs"].items():
            a.astype(a.dtype.newbyteorder("<")).tofile(work / f"{c['stem']}.{suffix}")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(work)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and r.stderr == "", r.stderr[-4000:]
    assert [l[4:] for l in r.stdout.splitlines() if l.startswith("ran ")] == [c["stem"] for c in cs]
    assert f"cases {len(cs)}\n" in r.stdout
    compared = 0
    for c in cs:
        for suffix, want in c["want"].items():
            got = np.fromfile(work / f"{c['stem']}.{suffix}", "<f4")
            assert got.size == want.size, (c["stem"], suffix, got.size, want.size)
            _eq(got.reshape(want.shape), want, f"{build} {c['stem']} {suffix}")
        for suffix in ("agg.f32", "best.f32", "disp.f32"):           # an output that was not requested is not written
            if c["line"].startswith("sgm ") and suffix not in c["want"]:
                assert not (work / f"{c['stem']}.{suffix}").exists(), (c["stem"], suffix)
        compared += 1
    assert compared == len(cs)
