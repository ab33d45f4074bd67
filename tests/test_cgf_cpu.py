"""The numpy reference of the colour-guided filter (tests/cgf_ref.py) on its own: against a float64 direct-sum filter that uses
no integral image and np.linalg.inv, on the isoluminant edge the feature exists for, and on its edge cases; the argument
checks of the entries that need no GPU to fail.  No GPU.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import stereo_matching_cuda_amd as smx
from stereo_matching_cuda_amd import _lib

import cgf_ref as ref

# The largest |q_ref - q_f64| over the seeded cases below, relative to the cost range (8), as measured: 1.620e-3, at 129 x 70,
# radius 1, eps 0.5 -- a 3 x 3 window of a noise guide, where the f32 integrals of I_c I_c' (up to 5.9e8, one ulp = 32 .. 64)
# leave an error of a few units in a variance that eps = 0.5 does not dominate; every case with radius >= 9 or eps 6.5025 stays
# below 2e-5.  The cases are seeded, so the deviation is deterministic; the factor of two covers another numpy build only
# (DESIGN.md 4.3g).
MEASURED_DEVIATION = 1.620e-3
COST_RANGE = 8.0

CASES = [  # (w, h, D, radius, eps, seed)
    (1, 1, 1, 9, 6.5025, 1), (2, 1, 3, 1, 6.5025, 2), (1, 7, 2, 9, 0.5, 3), (19, 40, 3, 12, 6.5025, 4), (65, 3, 2, 1, 0.5, 5),
    (64, 4, 2, 0, 6.5025, 6), (63, 5, 2, 9, 6.5025, 7), (129, 70, 3, 9, 6.5025, 8), (129, 70, 2, 12, 0.5, 9),
    (129, 70, 2, 1, 0.5, 10),
]


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _window_mean(x, radius):
    """float64 mean over the clamped window by direct summation of shifted copies; x: (..., h, w)"""
    h, w = x.shape[-2:]
    acc = np.zeros(x.shape, np.float64)
    cnt = np.zeros((h, w), np.float64)
    ry, rx = min(radius, h - 1), min(radius, w - 1)
    for dy in range(-ry, ry + 1):
        ys, yd = slice(max(dy, 0), h + min(dy, 0)), slice(max(-dy, 0), h + min(-dy, 0))
        for dx in range(-rx, rx + 1):
            xs, xd = slice(max(dx, 0), w + min(dx, 0)), slice(max(-dx, 0), w + min(-dx, 0))
            acc[..., yd, xd] += x[..., ys, xs]
            cnt[yd, xd] += 1
    return acc / cnt


def direct_f64(rgb, cost, radius, eps):
    """The colour guided filter of He et al. in float64: window sums, np.linalg.inv of Sigma + eps I."""
    I = rgb[:, :, :3].astype(np.float64).transpose(2, 0, 1)                     # (3, h, w)
    p = cost.astype(np.float64)                                                  # (D, h, w)
    mu = _window_mean(I, radius)
    second = _window_mean(I[:, None] * I[None, :], radius)                      # (3, 3, h, w)
    sigma = second - mu[:, None] * mu[None, :] + eps * np.eye(3)[:, :, None, None]
    inv = np.linalg.inv(sigma.transpose(2, 3, 0, 1)).transpose(2, 3, 0, 1)      # (3, 3, h, w)
    mp = _window_mean(p, radius)
    mip = _window_mean(I[:, None] * p[None, :], radius)                         # (3, D, h, w)
    cov = mip - mu[:, None] * mp[None, :]
    a = np.einsum("ijyx,jdyx->idyx", inv, cov)
    b = mp - np.einsum("idyx,iyx->dyx", a, mu)
    return np.einsum("idyx,iyx->dyx", _window_mean(a, radius), I) + _window_mean(b, radius)


def _case(w, h, D, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8), (rng.random((D, h, w)) * COST_RANGE).astype(np.float32)


def test_reference_against_a_float64_direct_sum_filter():
    worst = 0.0
    for w, h, D, radius, eps, seed in CASES:
        rgb, cost = _case(w, h, D, seed)
        q = ref.aggregate(rgb, cost, radius, eps)
        dev = float(np.abs(q.astype(np.float64) - direct_f64(rgb, cost, radius, eps)).max()) / COST_RANGE
        print(f"{w}x{h}x{D} r{radius} eps{eps}: |q_ref - q_f64| / range = {dev:.3e}")
        worst = max(worst, dev)
    print(f"largest deviation {worst:.3e}")
    assert worst <= 2 * MEASURED_DEVIATION


def test_integral_and_box_mean_are_the_oracles(orc):
    rng = np.random.default_rng(11)
    for w, h, radius in ((1, 1, 9), (2, 1, 0), (19, 40, 12), (65, 3, 1), (129, 70, 9)):
        img = (rng.random((h, w)) * 1000 - 300).astype(np.float32)
        S = ref.integral(img)
        assert np.array_equal(_bits(S), _bits(orc.integral(img)))
        assert np.array_equal(_bits(ref.box_mean(S, radius)), _bits(orc.box_mean(S, radius)))


def test_isoluminant_edge_is_kept_by_the_colour_guide_and_blurred_by_the_gray_one(orc):
    rgb, p, v = ref.isoluminant_scene(orc.gray)
    g = orc.gray(rgb)
    assert (g == v).all()                                         # no edge at all in the gray guide
    assert np.abs(rgb[0, 0].astype(int) - rgb[0, 63].astype(int)).tolist().count(0) <= 1
    q_rgb = ref.aggregate(rgb, p, 9, 6.5025)[0]
    q_gray = orc.guided_filter(g, p, 0, want_agg=True)[3][0]
    e_rgb = np.abs(q_rgb - p[0])[:, 31:33]
    e_gray = np.abs(q_gray - p[0])[:, 31:33]
    print("colour guide: max |q - p| next to the step", e_rgb.max(), " gray guide: min", e_gray.min())
    assert e_rgb.max() < 0.1
    assert e_gray.min() > 0.3


def test_flat_guide_gives_the_double_box_blur_bit_for_bit():
    # a colour of powers of two: every sum and product of the guidance is exact, so Sigma = eps I and a = 0 exactly
    rng = np.random.default_rng(21)
    for w, h, radius in ((19, 40, 12), (65, 9, 1), (129, 70, 9)):
        rgb = np.empty((h, w, 3), np.uint8)
        rgb[:] = (128, 64, 32)
        cost = (rng.random((2, h, w)) * COST_RANGE).astype(np.float32)
        I, mu, inv = ref.guidance(rgb, radius, 6.5025)
        for k, want in zip(range(6), (1, 0, 0, 1, 0, 1)):
            assert np.array_equal(inv[k], np.full((h, w), np.float32(want / 6.5025), np.float32)), k
        q = ref.aggregate(rgb, cost, radius, 6.5025)
        for z in range(2):
            bb = ref.box_mean(ref.integral(ref.box_mean(ref.integral(cost[z]), radius)), radius)
            assert np.array_equal(_bits(q[z]), _bits(bb))


def test_channels_3_and_4_give_the_same_bits():
    rgb, cost = _case(33, 9, 2, 31)
    rgba = np.concatenate((rgb, np.random.default_rng(32).integers(0, 256, (9, 33, 1), dtype=np.uint8)), axis=2)
    assert np.array_equal(_bits(ref.aggregate(rgb, cost, 3, 0.5)), _bits(ref.aggregate(rgba, cost, 3, 0.5)))


def test_states_are_those_of_the_streaming_passes():
    """keys / nbr / uq of cgf_ref.states are the definitions the _nbr and _uq entries are held to (subpix_ref, uniq_ref)."""
    import subpix_ref
    import uniq_ref
    rgb, cost = _case(21, 6, 7, 41)
    q = ref.aggregate(rgb, cost, 2, 6.5025)
    st = ref.states(q)
    z, lo, hi, last = subpix_ref.brute_state(q, [(0, 3), (3, 7)], chunk=2)
    assert np.array_equal(st["z"], z)
    for a, b in zip(st["nbr"], (lo, hi, last)):
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])
    key, sec, rest, last, _ = uniq_ref.emulate(q[:, 2, 5], [3, 4])
    assert key == st["keys"][2, 5] and _bits(sec) == _bits(st["uq"][0, 2, 5]) and _bits(rest) == _bits(st["uq"][1, 2, 5])


# ---------------------------------------------------------------------------------------------
# the CPU twin (host/cpu_twins.cpp colour_guided_filterOnCPU: what `smx_main --guidance rgb --host-compare` trusts)
# ---------------------------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "stereo_matching_cuda_amd", "host")
BUILDS = {
    "plain": ["-O2"],
    # the flags of test_host_twins_cpu.py
    "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fsanitize=float-cast-overflow", "-fno-sanitize-recover=all",
                  "-fno-omit-frame-pointer"],
}
TWIN_CASES = [  # (w, h, channels, D, dmin, radius, eps, want_agg, seed)
    (1, 1, 3, 1, 0, 9, 6.5025, 1, 1), (2, 1, 4, 3, -2, 1, 6.5025, 1, 2), (1, 7, 3, 2, 0, 9, 0.5, 0, 3),
    (19, 40, 3, 5, -4, 12, 6.5025, 1, 4), (65, 3, 4, 4, 0, 0, 0.5, 1, 5), (33, 66, 3, 2, -1, 9, 6.5025, 1, 6),
    (40, 9, 3, 3, 0, 2, 0.0, 1, 7),
]


def _twin_case(k, w, h, ch, D, dmin, radius, eps, want_agg, seed):
    rng = np.random.default_rng(seed)
    rgb = rng.integers(0, 256, (h, w, ch), dtype=np.uint8)
    if eps == 0.0:
        rgb[:] = rgb[0, 0]                                       # a flat guide without eps: det = 0, 0 / 0 everywhere
    cost = (rng.random((D, h, w)) * COST_RANGE).astype(np.float32)
    best, disp = smx.init_wta(h, w)
    best[rng.random((h, w)) < 0.2] = np.float32(0.5)             # IN/OUT: some pixels come in with a winner that mostly stays
    disp[best == np.float32(0.5)] = 99
    with np.errstate(all="ignore"):
        q = ref.aggregate(rgb, cost, radius, eps)
    wb, wd = best.copy(), disp.copy()
    for z in range(D):                                           # dispSelect: if (best >= q) { dmap = dmin + z; best = q; }
        with np.errstate(invalid="ignore"):
            take = wb >= q[z]
        wb, wd = np.where(take, q[z], wb), np.where(take, np.float32(dmin + z), wd)
    want = {"best.f32": wb, "disp.f32": wd}
    if want_agg:
        want["agg.f32"] = q
    stem = f"case{k}"
    return {"line": f"cgf {stem} {w} {h} {ch} {D} {dmin} {radius} {eps!r} {want_agg}", "stem": stem, "want": want,
            "inputs": {"rgb.u8": rgb, "cost.f32": cost, "best_in.f32": best, "disp_in.f32": disp}}


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_cpu_twin_equals_the_reference(build, tmp_path):
    cs = [_twin_case(k, *c) for k, c in enumerate(TWIN_CASES)]
    exe = str(tmp_path / "host_cgf_check")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off"] + BUILDS[build] +
                          ["-I" + os.path.join(ROOT, "include"), "-I" + HOST, os.path.join(ROOT, "tests", "host_cgf_check.cpp"),
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
    assert f"cases {len(cs)}\n" in r.stdout
    for c in cs:
        for suffix, want in c["want"].items():
            got = np.fromfile(work / f"{c['stem']}.{suffix}", "<f4").reshape(want.shape)
            both_nan = np.isnan(got) & np.isnan(want)
            same = (_bits(got) == _bits(want)) | both_nan
            assert same.all(), f"{c['line']}: {suffix}: {(~same).sum()} of {same.size} elements differ"


def test_argument_checks_of_the_entries():
    L = smx.lib()
    P = smx.default_params()
    assert L.smx_cgf_workspace_bytes(0, 5, 1, 1) == 0 and L.smx_cgf_workspace_bytes(5, 5, 0, 1) == 0
    assert L.smx_cgf_workspace_bytes(5, 5, 1, 3) == 0 and L.smx_cgf_workspace_bytes(5, 70000, 1, 1) == 0
    n = 7 * 5 * 4
    assert L.smx_cgf_workspace_bytes(7, 5, 1, 1) == 255 + 18 * n and L.smx_cgf_workspace_bytes(7, 5, 1, 2) == 255 + 36 * n
    assert L.smx_cgf_workspace_bytes(7, 5, 3, 2) == 255 + 2 * (9 + 24) * n
    rgb = np.zeros((5, 7, 3), np.uint8)
    cost = np.zeros((2, 5, 7), np.float32)
    best, dmap = smx.init_wta(5, 7)
    args = lambda **kw: [kw.get("p", C.byref(P)), kw.get("rgb", rgb.ctypes.data), kw.get("ch", 3),
                         kw.get("cost", cost.ctypes.data), kw.get("best", best.ctypes.data), dmap.ctypes.data, None,
                         kw.get("w", 7), kw.get("h", 5), kw.get("D", 2), 0]
    for bad in (dict(p=None), dict(rgb=None), dict(cost=None), dict(best=None), dict(ch=2), dict(ch=5), dict(w=0), dict(h=0),
                dict(D=0)):
        assert L.smx_colour_guided_filter(*args(**bad)) == -1, bad
    Q = smx.default_params()
    Q.radius = -1
    assert L.smx_colour_guided_filter(*args(p=C.byref(Q))) == -1
    one = C.c_void_p(256)           # (never dereferenced: every call below fails its checks first)
    dev = lambda **kw: [kw.get("p", C.byref(P)), kw.get("rl", one), kw.get("rr", one), kw.get("ch", 3), kw.get("cl", one),
                        kw.get("cr", one), kw.get("w", 7), kw.get("h", 5), kw.get("s0", 0), kw.get("s1", 2),
                        kw.get("keys", one), None, None, None, kw.get("ws", one), kw.get("wsb", 1 << 20), None]
    for bad in (dict(p=None), dict(ch=1), dict(w=0), dict(h=65536), dict(s0=-1), dict(s0=2), dict(keys=None),
                dict(rl=None, rr=None, cl=None, cr=None), dict(rl=None), dict(cr=None), dict(p=C.byref(Q))):
        assert L.smx_dev_cgf_wta_pair(*dev(**bad)) == -1, bad
    assert L.smx_dev_cgf_wta_pair(*dev(wsb=L.smx_cgf_workspace_bytes(7, 5, 1, 2) - 1)) == -3
    assert L.smx_dev_cgf_wta_pair(*dev(ws=None)) == -3
    assert b"workspace" in L.smx_last_error()
    with pytest.raises(ValueError):
        smx.colour_guided_filter(np.zeros((5, 7), np.uint8), cost, best, dmap, 0)
    with pytest.raises(ValueError):
        smx.colour_guided_filter(rgb, cost[:, :4], best, dmap, 0)
