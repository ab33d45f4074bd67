"""The uniqueness filter without a GPU: the streaming second-best cost against its brute-force definition, the test's rule, the
host-only argument checks of the new entries, and what the filter is good for on a scene with a periodic-texture band.

  recurrence    tests/uniq_ref.emulate (plain Python) AND the library's own WtaRunUq (smx_common.h, through the host hook
                smx_debug_uq_run) over every chunk split for D = 1, 2, 3, 4 and random splits at D = 9, 17, against uniq_ref.second_best, which
                computes sec from the final winner by the definition.  Bit for bit.
  rule          uniq_rejects (the filter kernel's pixel, through smx_debug_uniq_test) against uniq_ref.rejects / margin.
  host twin     uniqueness_onCPU (host/cpu_twins.cpp: sec by brute force from the volume, in C++) through the stand-alone
                tests/uniq_check.cpp, plain and under the host sanitizers, against uniq_ref.
  usefulness    references only (oracle + speckle_ref + uniq_ref): see test_usefulness_on_a_periodic_band.

Mutations this file was checked against (each makes at least one test fail): `<=` for `<` in the test's comparison; `z* + 1` for
`z* + 2`; a dropped `rest` update; `sec = last` instead of `sec = rest` on a take.
"""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import stereo_matching_cuda_amd as smx
from stereo_matching_cuda_amd import _lib

import uniq_ref as ref

F32 = np.float32
SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 2.0, 3.0, -2.5, 1e-45, 3.4e38], F32)


@pytest.fixture(scope="module")
def so():
    if not smx._lib.os.path.exists(_lib.SO_PATH):
        smx.build()
    L = C.CDLL(_lib.SO_PATH)
    L.smx_debug_uq_run.restype = C.c_int
    L.smx_debug_uq_run.argtypes = [C.POINTER(C.c_float), C.c_int, C.c_uint32, C.POINTER(C.c_int64), C.POINTER(C.c_float)]
    L.smx_debug_uniq_test.restype = C.c_int
    L.smx_debug_uniq_test.argtypes = [C.c_int64, C.c_float, C.c_float, C.POINTER(C.c_float)]
    return L


def _columns(D, count, seed):
    """count pixels of D slices: small integers (ties), specials (+-0, +-inf, NaN, negatives), NaN runs, all-NaN pixels"""
    rng = np.random.default_rng(seed)
    cols = []
    for i in range(count):
        kind = i % 6
        if kind == 0:
            c = rng.integers(0, 3, D).astype(F32)                               # frequent exact ties
        elif kind == 1:
            c = SPECIAL[rng.integers(0, len(SPECIAL), D)]
        elif kind == 2:
            c = rng.standard_normal(D).astype(F32)
        elif kind == 3:
            c = rng.integers(-2, 3, D).astype(F32)
            a = int(rng.integers(0, D))
            c[a:a + int(rng.integers(1, D + 1))] = np.nan                       # a NaN run
        elif kind == 4:
            c = np.where(rng.random(D) < 0.5, F32(0.0), F32(-0.0)).astype(F32)   # +-0 only
            if D > 2 and rng.random() < 0.5:
                c[int(rng.integers(0, D))] = 1.0
        else:
            c = np.full(D, np.nan, F32) if i % 12 == 5 else np.where(rng.integers(0, 2, D) > 0, F32(np.inf), F32(0)).astype(F32)
        cols.append(c)
    return np.stack(cols, axis=1).reshape(D, 1, count)                            # q[D][1][count]


def _bits(x):
    x = np.asarray(x, F32)
    return np.where(np.isnan(x), np.uint32(0x7FC00000), x.view(np.uint32))      # (any NaN is a NaN)


def _lib_run(so, col, chunks, s_begin):
    key = C.c_int64(ref.IDENT)
    state = (C.c_float * 3)(123.0, -7.0, 55.0)
    at = 0
    for n in chunks:
        part = np.ascontiguousarray(col[at:at + n], F32)
        assert so.smx_debug_uq_run(part.ctypes.data_as(C.POINTER(C.c_float)), n, s_begin + at, C.byref(key), state) == 0
        at += n
    return key.value, F32(state[0]), F32(state[1]), F32(state[2])


_SWEEPS = {}
DS = [1, 2, 3, 4, 9, 17]


def _sweep(so, D):
    """Every pixel of _columns(D) over its splits, both implementations against the definition; -> the counts of the inputs"""
    if D in _SWEEPS:
        return _SWEEPS[D]
    n = dict(last=0, first=0, before=0, after=0, ties=0, inf=0, allnan=0, cases=0)
    s_begin = 3 if D % 2 else 0
    q = _columns(D, 96 if D <= 6 else 240, 100 + D)
    full = np.concatenate([np.full((s_begin,) + q.shape[1:], -9.0, F32), q])     # (slices below s_begin are not seen)
    z, c0, sec, rest, last, zsec = (a[0] for a in ref.second_best(full, s_begin, s_begin + D))
    want_keys = ref.pack_keys(c0, z)
    rng = np.random.default_rng(D)
    for p in range(q.shape[2]):
        col = q[:, 0, p]
        if D <= 6:
            every = ref.splits(D)
        else:
            every = [[D], [1] * D]
            for _ in range(6):
                cuts = sorted(int(c) for c in rng.choice(np.arange(1, D), int(rng.integers(1, 5)), replace=False))
                every.append([b - a for a, b in zip([0] + cuts, cuts + [D])])
        for chunks in every:
            k, s, r, l, trace = ref.emulate(col, chunks, s_begin)
            for got in ((k, s, r, l), _lib_run(so, col, chunks, s_begin)):
                assert got[0] == want_keys[p], (D, p, chunks, col)
                assert _bits(got[1]) == _bits(sec[p]), ("sec", D, p, chunks, col, got[1], sec[p])
                assert _bits(got[2]) == _bits(rest[p]), ("rest", D, p, chunks, col, got[2], rest[p])
                assert _bits(got[3]) == _bits(last[p]), ("last", D, p, chunks, col)
            n["cases"] += 1
            if z[p] >= 0 and len(trace) > 1:
                n["last"] += any(b == z[p] for a, b, w in trace)
                n["first"] += any(a == z[p] for a, b, w in trace)
        n["before"] += int(0 <= zsec[p] < z[p])
        n["after"] += int(zsec[p] > z[p] >= 0)
        n["ties"] += int(z[p] >= 0 and zsec[p] >= 0 and sec[p] == c0[p])
        n["inf"] += int(z[p] >= 0 and np.isposinf(sec[p]))
        n["allnan"] += int(z[p] < 0)
    _SWEEPS[D] = n
    return n


@pytest.mark.parametrize("D", DS)
def test_recurrence_equals_the_definition(so, D):
    _sweep(so, D)


def test_the_inputs_met_their_conditions(so):
    total = {k: sum(_sweep(so, D)[k] for D in DS) for k in ("last", "first", "before", "after", "ties", "inf", "allnan", "cases")}
    for k, v in total.items():
        assert v > 0, (k, total)
    # 96 pixels x 2^(D-1) splits for D = 1, 2, 3, 4 and 240 x 8 for D = 9, 17
    assert total["cases"] == 96 * (1 + 2 + 4 + 8) + 2 * 240 * 8, total


def test_rule_of_the_filter_kernel_pixel(so):
    """every clause: identity key; unknown s (+inf, NaN); negative, zero and infinite c0; s == c0 (a far tie); ratio 0;
    the boundary s - c0 == ratio * |c0| (not rejected: the comparison is strict)"""
    c0s = np.array([0.0, -0.0, 1.0, -1.0, 4.0, -4.0, 100.0, 1e-30, np.inf, -np.inf, 3.0e38], F32)
    secs = np.array([0.0, 1.0, 1.5, 2.0, 4.0, 5.0, 6.0, -3.0, -4.0, 100.0, 150.0, np.inf, -np.inf, np.nan, 3.4e38], F32)
    ratios = [0.0, 0.25, 0.5, 1.0, 1e-3, 17.0]
    n_rej = n_boundary = 0
    for c0, s, ratio in itertools.product(c0s, secs, ratios):
        for key in (ref.pack_key(c0, 5), ref.IDENT):
            has = np.array(key != ref.IDENT)
            cc = ref.unpack_key(key)[0] if has else ref.NAN
            m = C.c_float()
            got = so.smx_debug_uniq_test(key, float(s), ratio, C.byref(m))
            want = bool(ref.rejects(has, cc, s, ratio))
            assert got == int(want), (c0, s, ratio, key)
            assert _bits(F32(m.value)) == _bits(ref.margin(has, cc, s)), (c0, s, ratio, key)
            n_rej += want
            with np.errstate(invalid="ignore", over="ignore"):
                n_boundary += int(has and ratio > 0 and F32(s) - cc == F32(ratio) * abs(cc) and not want)
            if not has or ratio == 0 or not (s < np.inf):
                assert not want
    assert n_rej > 50 and n_boundary > 0
    # the boundary itself: c0 = 4, ratio 0.25 -> bound 1: s = 5 stays, the float just below goes
    m = C.c_float()
    assert so.smx_debug_uniq_test(ref.pack_key(4.0, 0), 5.0, 0.25, C.byref(m)) == 0 and m.value == 1.0
    assert so.smx_debug_uniq_test(ref.pack_key(4.0, 0), float(np.nextafter(F32(5.0), F32(0.0))), 0.25, C.byref(m)) == 1


def test_argument_checks_need_no_gpu():
    L = smx.lib()
    one = C.c_void_p(16)                        # (never dereferenced: the checks come first)
    for ratio in (float("nan"), -0.5, float("inf")):
        assert L.smx_dev_uniqueness(ratio, one, one, one, one, None, 4, 4, 0.0, -100.0, None) == -1
        assert b"bad argument" in L.smx_last_error()
        assert L.smx_uniqueness_filter(ratio, one, one, one, one, None, 4, 4, 0.0, -100.0) == -1
    for bad in range(4):
        ptrs = [one] * 4
        ptrs[bad] = None
        assert L.smx_dev_uniqueness(0.5, *ptrs, None, 4, 4, 0.0, -100.0, None) == -1
        assert L.smx_uniqueness_filter(0.5, *ptrs, None, 4, 4, 0.0, -100.0) == -1
    assert L.smx_dev_uniqueness(0.5, one, one, one, one, None, 0, 4, 0.0, -100.0, None) == -1
    assert L.smx_dev_uniqueness(0.5, one, one, one, one, None, 4, 0, 0.0, -100.0, None) == -1
    p = smx.default_params()
    # d_uq is what the entry is for; the cost pointers come both or not at all
    assert L.smx_dev_aggregate_wta_pair_uq(C.byref(p), one, one, None, None, 8, 4, 0, 0, 0, 2, one, None, None, one, 1 << 20,
                                           None, None, None) == -1
    assert L.smx_dev_aggregate_wta_pair_uq(C.byref(p), one, one, one, None, 8, 4, 0, 0, 0, 2, one, None, None, one, 1 << 20,
                                           None, one, None) == -1
    g = smx.default_sgm_params()
    assert L.smx_dev_sgm_wta_pair_uq(C.byref(g), one, one, 8, 4, 4, one, None, None, None, one, 1 << 20, None) == -1
    assert L.smx_dev_sgm_wta_pair_uq(C.byref(g), one, one, 8, 4, 4, one, None, None, one, None, 0, None) == -3      # SMX_E_WS
    with pytest.raises(ValueError):
        smx.uniqueness_filter(np.zeros((2, 3), np.int64), np.zeros((2, 2), F32), np.zeros((2, 3), F32), 0.5, 0, -100)


# ---------------------------------------------------------------------------------------------
# usefulness: references only
# ---------------------------------------------------------------------------------------------
W, H, D, SHIFT, PERIOD, AMP = 128, 72, 16, 5, 6, 4
BAND = slice(12, 60)
RATIO = 0.05            # about OpenCV's uniquenessRatio 5: 5 / (100 - 5)
SPECKLE = 50            # (the default 200 is for full-size images)


def _scene():
    """A random-texture pair at disparity -SHIFT (left labels) with a band of rows that holds stripes of period PERIOD plus
    independent noise of +-AMP in each view: inside the band the disparities -SHIFT - k * PERIOD match almost equally well,
    and the noise decides -- in patches, and often the same way in both views, so the LR check passes."""
    rng = np.random.default_rng(7)
    base = rng.integers(0, 256, (H, W + D)).astype(np.int64)
    stripes = (np.arange(W + D) % PERIOD < PERIOD // 2) * 150 + 40
    left, right = base[:, :W].copy(), base[:, SHIFT:SHIFT + W].copy()
    nb = BAND.stop - BAND.start
    left[BAND] = stripes[None, :W] + rng.integers(-AMP, AMP + 1, (nb, W))
    right[BAND] = stripes[None, SHIFT:SHIFT + W] + rng.integers(-AMP, AMP + 1, (nb, W))
    return np.clip(left, 0, 255).astype(np.uint8), np.clip(right, 0, 255).astype(np.uint8)


def test_usefulness_on_a_periodic_band():
    """References only (the oracle's pair, tests/speckle_ref.py, tests/uniq_ref.py), 128 x 72, D 16, dminl -15: true disparity
    -5 everywhere, rows 12 .. 59 striped with period 6.  Counted on the left map after LR check + speckle filter (max_size 50),
    over the pixels that still hold a label:
        without the filter        wrong 690    correct 7877
        with ratio 0.05           wrong   0    correct 6917   (kept-correct share 6917 / 7877 = 0.878)
    Strict improvement in wrong pixels, and the kept-correct share is held at what the references give: deterministic."""
    import oracle
    import speckle_ref
    Il, Ir = _scene()
    dminl = -(D - 1)
    want = oracle.stereo_pair(Il, Ir, D, dminl=dminl, dminr=0, want_agg=True)
    z, c0, sec = ref.second_best(want["aggl"])[:3]
    occ = want["occlusion"]
    unique, _ = ref.apply(occ, z >= 0, c0, sec, RATIO, dminl, dminl - 100)
    truth = F32(-SHIFT)

    def tally(m):
        m = speckle_ref.speckle_filter(m, float(dminl), float(dminl - 100), SPECKLE, 1.0)
        valid = ref.counts(m, dminl)
        return int((valid & (m != truth)).sum()), int((valid & (m == truth)).sum())
    wrong0, right0 = tally(occ)
    wrong1, right1 = tally(unique)
    print("usefulness: wrong, correct without", (wrong0, right0), "with", (wrong1, right1))
    assert wrong0 > 0, "the scene must leave wrong pixels behind LR check + speckle"
    assert wrong1 < wrong0 and 2 * wrong1 <= wrong0, "the filter removes most of them"
    assert 2 * right1 >= right0, "and keeps most correct pixels"
    assert (wrong0, right0, wrong1, right1) == (690, 7877, 0, 6917)
    assert right1 * 7877 >= 6917 * right0


# ---------------------------------------------------------------------------------------------
# the host twin (host/cpu_twins.cpp uniqueness_onCPU) as its own executable, plain and sanitized
# ---------------------------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "stereo_matching_cuda_amd", "host")
TWIN_BUILDS = {
    "plain": ["-O2"],
    # the flags of tests/test_host_twins_cpu.py
    "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fsanitize=float-cast-overflow", "-fno-sanitize-recover=all",
                  "-fno-omit-frame-pointer"],
}


def _hex(v):
    return "%08X" % int(np.array(v, F32).view(np.uint32))


def _twin_cases():
    """(line of cases.txt, stem, agg, disp, want out, want margin or None): the volumes of the sweep above as images of one row,
    a random-float volume, and a 1 x 1 x 1 one; ratios 0, 0.05, 0.25, 1; maps with markers and specials."""
    out = []
    disps = np.array([-15.0, -3.0, 0.0, -0.0, 2.5, -115.0, -16.0, -15.5, np.nan, np.inf, -np.inf, 3e9, -3e9], F32)
    vols = [(f"cols{D}", _columns(D, 96, 100 + D)) for D in (1, 2, 3, 4, 9, 17)]
    rng = np.random.default_rng(31)
    vols.append(("random", (rng.integers(0, 40, (12, 7, 19)) * F32(0.25)).astype(F32)))
    vols.append(("one", np.array([[[3.0]]], F32)))
    k = 0
    for name, q in vols:
        D, h, w = q.shape
        z, c0, sec = ref.second_best(q)[:3]
        for ratio in (0.0, 0.05, 0.25, 1.0):
            disp = disps[np.random.default_rng(k).integers(0, disps.size, (h, w))]
            want, margin = ref.apply(disp, z >= 0, c0, sec, ratio, -15.0, -115.0)
            want_margin = k % 3 != 0
            stem = f"uniq_{name}_r{k}"
            line = f"uniq {stem} {w} {h} {D} {_hex(ratio)} {_hex(-15.0)} {_hex(-115.0)} {int(want_margin)}"
            out.append((line, stem, q, disp, want, margin if want_margin else None))
            k += 1
    return out


@pytest.mark.parametrize("build", list(TWIN_BUILDS))
def test_host_twin_equals_the_reference(tmp_path, build):
    """tests/uniq_check.cpp over cpu_twins.cpp alone: exit status 0, a clean stderr (the sanitized build is the program itself,
    nothing preloaded), every output equal to uniq_ref's bits; the number of compared cases is asserted."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    cs = _twin_cases()
    exe = str(tmp_path / "uniq_check")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off"] + TWIN_BUILDS[build] +
                          ["-I" + os.path.join(ROOT, "include"), "-I" + HOST, os.path.join(ROOT, "tests", "uniq_check.cpp"),
                           os.path.join(HOST, "cpu_twins.cpp"), "-o", exe])
    work = tmp_path / "cases"
    work.mkdir()
    (work / "cases.txt").write_text("\n".join(c[0] for c in cs) + "\n")
    for line, stem, q, disp, want, margin in cs:
        q.astype("<f4").tofile(work / f"{stem}.agg.f32")
        disp.astype("<f4").tofile(work / f"{stem}.disp.f32")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(work)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stderr == "", r.stderr[-4000:]
    assert f"cases {len(cs)}\n" in r.stdout and len(cs) == 8 * 4
    compared = changed = 0
    for line, stem, q, disp, want, margin in cs:
        got = np.fromfile(work / f"{stem}.out.f32", "<f4").reshape(want.shape)
        assert np.array_equal(_bits(got), _bits(want)) and np.array_equal(got.view(np.uint32)[~np.isnan(want)],
                                                                          want.view(np.uint32)[~np.isnan(want)]), stem
        changed += int((_bits(want) != _bits(disp)).sum())
        if margin is not None:
            assert np.array_equal(_bits(np.fromfile(work / f"{stem}.margin.f32", "<f4").reshape(margin.shape)), _bits(margin)), stem
        else:
            assert not (work / f"{stem}.margin.f32").exists()
        compared += 1
    assert compared == 32 and changed > 100
