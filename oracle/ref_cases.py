"""The one table of cases that pin the oracle and the HIP kernels to the reference's own code (TEST INFRASTRUCTURE ONLY).

oracle/ref_build.py builds the reference once per distinct macro set of this table, generates each case's inputs with
`inputs(case)`, runs the reference and records the results (tests/golden/ref_cases/<name>.npz).  The tests import this module
to regenerate the identical inputs: nothing here reads the reference or oracle/_ref.

A case: name, macros (the #define lines of SystemIncludes.h it is built with), mode (pair / gf / occ / gray / wm, the modes of
oracle/ref_driver.cpp), w, h, seed, recipe and what the recipe needs.  `axes` names the axis values of the issue a case stands
for; oracle/REF_CASES.md is checked against it.
"""
import os

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# SystemIncludes.h:10-14, 21-24.  EPS and ALPHA are written as double literals and the others as int literals, like the
# reference's own lines: the literal's type is part of the arithmetic (guidedFilter.cu:350 adds EPS in double).
DEFAULTS = dict(D_MIN=-15, D_MAX=0, RADIUS=9, EPS=6.5025, ALPHA=0.9, TH_color=7, TH_grad=2, D_LR=0)
MACRO_ORDER = ("D_MIN", "D_MAX", "RADIUS", "EPS", "ALPHA", "TH_color", "TH_grad", "D_LR")


def macros(**kw):
    m = dict(DEFAULTS)
    m.update(kw)
    return m


def macro_text(key, value):
    return repr(float(value)) if key in ("EPS", "ALPHA") else str(int(value))


def variant(m):
    """Name of the build of one macro set."""
    return "_".join(macro_text(k, m[k]).replace("-", "m").replace(".", "p") for k in MACRO_ORDER)


def size_d(m):
    return m["D_MAX"] - m["D_MIN"] + 1


# ---- the macro sets --------------------------------------------------------------------------------------------------
M_DEF = macros()
M_R0 = macros(D_MIN=-23, RADIUS=0, ALPHA=0.5, TH_color=3, TH_grad=1, EPS=1.0)      # var + eps can be 0: NaN slices
M_R1 = macros(D_MIN=-23, RADIUS=1, EPS=0.5, D_LR=1)
M_R3 = macros(D_MIN=-23, RADIUS=3, ALPHA=0.1)
M_R4 = macros(D_MIN=-23, RADIUS=4, EPS=100.0, TH_color=29, TH_grad=7, D_LR=2)
M_R5 = macros(D_MIN=-30, D_MAX=7, RADIUS=5, ALPHA=0.25, TH_color=20, TH_grad=5, EPS=0.01)
M_R9 = macros(D_MIN=-23)
M_R12 = macros(D_MIN=-23, RADIUS=12)
M_BORDER = macros(D_MIN=-400, D_MAX=-377)                                          # every partner outside a 210-wide image
M_D70 = macros(D_MIN=-69)
M_KITTI = macros(D_MIN=-31)
# one axis away from the defaults
M_EPS1 = macros(EPS=1.0)
M_EPS05 = macros(EPS=0.5)
M_EPS100 = macros(EPS=100.0)
M_A05 = macros(ALPHA=0.5)
M_TH20 = macros(TH_color=20, TH_grad=5)
M_LR2 = macros(D_LR=2)
# ranges the command line of smx_main can ask for and no other set has: one that does not end at zero, one that crosses
# zero (its right view starts at -6, its positive-disparity outputs hold negative values), one with a single label
M_NZ = macros(D_MIN=-40, D_MAX=-6)
M_X0 = macros(D_MIN=-5, D_MAX=6)
M_ONE = macros(D_MIN=-4, D_MAX=-4)

CASES = []


def _case(name, m, mode, w, h, seed, recipe, axes=(), **extra):
    assert all(c["name"] != name for c in CASES), name
    c = dict(name=name, macros=m, mode=mode, w=w, h=h, seed=seed, recipe=recipe, axes=tuple(axes))
    c.update(extra)
    CASES.append(c)


def _mx(m):
    """The axis values a macro set stands for."""
    return (f"radius={m['RADIUS']}", f"eps={macro_text('EPS', m['EPS'])}", f"alpha={macro_text('ALPHA', m['ALPHA'])}",
            f"th=({m['TH_color']},{m['TH_grad']})", f"range=({m['D_MIN']},{m['D_MAX']})", f"d_lr={m['D_LR']}")


# ---- pair mode -------------------------------------------------------------------------------------------------------
_case("tsukuba", M_DEF, "pair", 384, 288, 0, "tsukuba", _mx(M_DEF) + ("tsukuba",), channels=3)
_case("r0_210x150", M_R0, "pair", 210, 150, 100, "quant", _mx(M_R0) + ("content=quant", "shape=210x150"))
_case("r1_210x150", M_R1, "pair", 210, 150, 101, "shift", _mx(M_R1) + ("content=shift", "shape=210x150"))
_case("r3_210x150", M_R3, "pair", 210, 150, 103, "shift", _mx(M_R3) + ("shape=210x150",))
_case("r4_210x150", M_R4, "pair", 210, 150, 104, "noise", _mx(M_R4) + ("content=noise", "shape=210x150"))
_case("r5_210x150", M_R5, "pair", 210, 150, 105, "shift", _mx(M_R5) + ("shape=210x150",))
_case("r9_210x150", M_R9, "pair", 210, 150, 109, "shift", _mx(M_R9) + ("shape=210x150",))
_case("r12_210x150", M_R12, "pair", 210, 150, 112, "shift", _mx(M_R12) + ("shape=210x150",))
_case("border_210x150", M_BORDER, "pair", 210, 150, 120, "noise", _mx(M_BORDER) + ("shape=210x150",))
_case("d70_129x70", M_D70, "pair", 129, 70, 121, "shift", _mx(M_D70) + ("shape=129x70",))
_case("kitti_1242x375", M_KITTI, "pair", 1242, 375, 122, "shift", _mx(M_KITTI) + ("shape=1242x375",),
      hash_only=("bestl", "bestr"))
for _name, _m, _recipe, _seed in (("eps1", M_EPS1, "quant", 130), ("eps05", M_EPS05, "shift", 131),
                                  ("eps100", M_EPS100, "shift", 132), ("alpha05", M_A05, "shift", 133),
                                  ("th20_5", M_TH20, "shift", 134), ("dlr2", M_LR2, "shift", 135)):
    _case(f"{_name}_129x70", _m, "pair", 129, 70, _seed, _recipe, _mx(_m) + ("shape=129x70", f"content={_recipe}"))
# images smaller than the (2 RADIUS + 1)^2 window in one or both directions, ragged, and the two smallest
_SMALL = ((129, 70), (19, 40), (20, 20), (64, 9), (2, 1), (1, 1))
for _tag, _m in (("r9", M_DEF), ("r0", M_R0), ("r3", M_R3), ("r12", M_R12)):
    for _i, (_w, _h) in enumerate(_SMALL):
        _case(f"{_tag}_{_w}x{_h}", _m, "pair", _w, _h, 200 + 10 * _m["RADIUS"] + _i, "quant" if _tag == "r0" else "shift",
              (f"radius={_m['RADIUS']}", f"shape={_w}x{_h}"))
for _tag, _m in (("r1", M_R1), ("r4", M_R4), ("r5", M_R5)):
    _case(f"{_tag}_20x20", _m, "pair", 20, 20, 400 + _m["RADIUS"], "shift", (f"radius={_m['RADIUS']}", "shape=20x20"))

# RGB(A) pairs for the drop-in main (tests/test_gpu_main_cases.py): smx_main converts RGB itself and takes only the range
# from its command line, so every other macro is at its default.  `shift`: columns the right view is moved by, one value per
# horizontal band of the image (the true left disparity of a band is -shift).  The seeds of the two smallest cases were searched
# for what tests/test_gpu_main_cases.py asserts of the recordings: cli_2x1 has one occluded pixel and two labels per view, and
# slice 0 of cli_19x40's right cost volume has its smallest value in its first pixel alone (a wrapped 8-bit level)
for _name, _m, _w, _h, _ch, _seed, _shift, _extra in (
        ("cli_d70_129x70", M_D70, 129, 70, 3, 500, (9, 31), {}),
        ("cli_r9_210x150", M_R9, 210, 150, 4, 501, (9, 17), {}),
        ("cli_19x40", M_DEF, 19, 40, 3, 2690, (6, 2), {}),
        ("cli_2x1", M_DEF, 2, 1, 3, 24, (1,), {}),
        ("cli_kitti_1242x375", M_KITTI, 1242, 375, 3, 504, (9, 25), {"hash_only": ("bestl", "bestr")}),
        ("cli_nz_210x150", M_NZ, 210, 150, 3, 505, (9, 30), {}),
        ("cli_x0_210x150", M_X0, 210, 150, 3, 506, (3, -4), {}),
        ("cli_one_64x9", M_ONE, 64, 9, 3, 507, (4,), {})):
    _case(_name, _m, "pair", _w, _h, _seed, "rgb", (f"range=({_m['D_MIN']},{_m['D_MAX']})", f"shape={_w}x{_h}",
                                                    f"cli=RGB input, {_ch} channels"), channels=_ch, shift=_shift, **_extra)

# ---- gf mode: compute_guided_filter on a supplied volume with supplied presets ------------------------------------------
_case("gf_fresh", M_DEF, "gf", 45, 37, 11, "gf_random", ("gf=fresh presets",), size_d=6, dmin=-5)
_case("gf_inout", M_DEF, "gf", 45, 37, 11, "gf_inout", ("gf=presets below some q", "gf=ties with the preset on alternate rows"),
      size_d=6, dmin=-5, needs="gf_fresh")
_case("gf_ties5", M_DEF, "gf", 40, 21, 13, "gf_ties5", ("gf=[c, c+1, c, c+2, c]",), size_d=5, dmin=0)
# costs costVolume.cu:187 never produces (negative, -0, below 2^-60): plain arithmetic for the reference; the comb walker's value
# check sends such a call to its queued fall-back
_case("gf_odd_costs", M_DEF, "gf", 45, 37, 12, "gf_odd_costs", ("gf=costs outside the comb walker's value check",), size_d=6,
      dmin=-5)

# ---- occ mode ---------------------------------------------------------------------------------------------------------
for _w in (1, 63, 64, 65, 200, 1242):
    _case(f"occ_fill_w{_w}", M_DEF, "occ", _w, 15, _w, "fill_adversarial",
          (f"fill width={_w}", "fill=integer", "fill=non-integer", "fill=fully occluded row", "fill=runs at each border"),
          d_occlusion=-120, vmin=-20.0)
for _tag, _m in (("dlr0", M_DEF), ("dlr1", M_R1), ("dlr2", M_R4)):
    _case(f"occ_detect_{_tag}", _m, "occ", 90, 11, 17, "detect_random", (f"detect d_lr={_m['D_LR']}",),
          d_occlusion=-129, vmin=-29.0)

# ---- gray mode --------------------------------------------------------------------------------------------------------
_case("gray_lattice", M_DEF, "gray", 52 ** 3, 1, 0, "gray_lattice", ("gray=5-step lattice",), channels=3)
_case("gray_rgba", M_DEF, "gray", 65, 33, 5, "gray_random", ("gray=4 channels",), channels=4)

# ---- wm mode: write_mat, the float -> 8-bit normaliser in front of the PNG writer (main.cu:13-35) --------------------------
# Its minimum skips every element that raises the running maximum (`else if`, main.cu:22), so what it does depends on the
# order of the values, not only on their range.
for _recipe, _what in (("wm_random", "random map"), ("wm_first_min", "first element is the global minimum (a negative level wraps)"),
                       ("wm_increasing", "strictly increasing (min stays 150000000)"), ("wm_decreasing", "strictly decreasing"),
                       ("wm_two_valued", "two values"), ("wm_occlusion", "integer labels with the d_lo - 100 sentinel scattered"),
                       ("wm_constant", "constant map")):
    _case(_recipe, M_DEF, "wm", 331, 1, 600, _recipe, (f"wm={_what}",))

BY_NAME = {c["name"]: c for c in CASES}
VARIANTS = {}
for _c in CASES:
    VARIANTS.setdefault(variant(_c["macros"]), _c["macros"])


# ---- inputs -----------------------------------------------------------------------------------------------------------
def _pair_images(c):
    w, h, D = c["w"], c["h"], size_d(c["macros"])
    rng = np.random.default_rng(c["seed"])
    if c["recipe"] == "tsukuba":
        g = np.load(os.path.join(_ROOT, "tests", "golden", "tsukuba_golden.npz"))
        return g["tsukuba0"], g["tsukuba1"]
    if c["recipe"] == "rgb":
        # every channel is noise of its own; the right view is the left one moved by shift[b] columns in band b; with four
        # channels the alpha of each view is noise too (the conversion must ignore it)
        shifts = c["shift"]
        pad = max(abs(s) for s in shifts)
        base = rng.integers(0, 256, size=(h, w + 2 * pad, 3), dtype=np.uint8)
        left = base[:, pad:pad + w]
        right = np.empty_like(left)
        for rows, s in zip(np.array_split(np.arange(h), len(shifts)), shifts):
            right[rows] = base[rows, pad + s:pad + s + w]
        if c["channels"] == 4:
            left, right = (np.concatenate([v, rng.integers(0, 256, size=(h, w, 1), dtype=np.uint8)], -1) for v in (left, right))
        return np.ascontiguousarray(left), np.ascontiguousarray(right)
    if c["recipe"] == "noise":
        return (rng.integers(0, 256, size=(h, w), dtype=np.uint8), rng.integers(0, 256, size=(h, w), dtype=np.uint8))
    # "shift": the right view is the left one moved by `shift` columns, so the true disparity lies inside every range that
    # holds -shift; "quant": the same in multiples of 64 (flat patches: zero costs, exact ties, tiny sums)
    shift = min(9, w // 3)
    base = rng.integers(0, 256, size=(h, w + D + 8), dtype=np.uint8)
    if c["recipe"] == "quant":
        base = (base // 64 * 64).astype(np.uint8)
    else:
        assert c["recipe"] == "shift", c["recipe"]
    return np.ascontiguousarray(base[:, :w]), np.ascontiguousarray(base[:, shift:shift + w])


def _wta_presets(h, w):
    return np.full((h, w), 0x7F7F7F7F, np.uint32).view(np.float32), np.zeros((h, w), np.float32)


def inputs(c, needs=None):
    """The case's input arrays by the driver's file stem.  `needs`: the recorded outputs (fixture) of the case c["needs"]."""
    w, h = c["w"], c["h"]
    rng = np.random.default_rng(c["seed"])
    mode, recipe = c["mode"], c["recipe"]
    if mode == "pair":
        left, right = _pair_images(c)
        return {"left": left, "right": right}
    if mode == "gf":
        I = rng.integers(0, 256, size=(h, w), dtype=np.uint8)
        if recipe == "gf_ties5":                # duplicate slices: exact ties in q between slices 0, 2 and 4
            one = (rng.random((1, h, w), dtype=np.float32) * 2.5).astype(np.float32)
            cost = np.concatenate([one, one + 1, one, one + 2, one], 0)
        else:
            cost = (rng.random((c["size_d"], h, w), dtype=np.float32) * 2.5).astype(np.float32)
        if recipe == "gf_odd_costs":
            cost[1, 7, 20] = np.float32(-0.75)
            cost[2, 10, 10] = np.float32(-0.0)
            cost[4, h - 1, 0] = np.float32(2.0 ** -70)
        best, dmap = _wta_presets(h, w)
        if recipe == "gf_inout":                # a preset below some q everywhere; on even rows the preset IS the smallest q
            fresh = needs["best"]
            best = np.full((h, w), np.median(fresh).astype(np.float32), np.float32)
            best[::2] = fresh[::2]
            dmap = np.full((h, w), 77, np.float32)
        return {"I": I, "cost": cost, "best": best, "dmap": dmap}
    if mode == "occ":
        if recipe == "fill_adversarial":
            hb = h // 3
            vmin = c["vmin"]
            d = rng.integers(int(vmin), 1, size=(hb, w)).astype(np.float32)
            d[rng.random((hb, w)) < 0.6] = c["d_occlusion"]
            d[0, :] = c["d_occlusion"]                      # a fully occluded row
            d[1, : w // 2] = c["d_occlusion"]               # a run touching the left border
            d[2, w // 2:] = c["d_occlusion"]                # a run touching the right border
            # non-integer values: (int)v >= vMin decides "occluded", v >= vMin decides "valid" (occlusion.cu:140-142, :152).
            # + fraction: every valid pixel stays valid; - fraction: vMin - f is neither occluded nor valid
            up = d + rng.random((hb, w)).astype(np.float32) * np.float32(0.9)
            down = d - rng.random((hb, w)).astype(np.float32) * np.float32(0.9)
            return {"dl": np.concatenate([d, up, down], 0).astype(np.float32)}
        assert recipe == "detect_random"
        D = 30
        dl = -rng.integers(0, D, size=(h, w)).astype(np.float32)
        dr = rng.integers(0, D, size=(h, w)).astype(np.float32)
        half = rng.random((h, w)) < 0.25                    # abs(d + dR) compares in float: halves sit between the d_lr steps
        dr[half] += np.float32(0.5)
        return {"dl": dl, "dr": dr}
    if mode == "wm":
        n = w * h
        if recipe == "wm_constant":
            return {"mat": np.full(n, -7.0, np.float32)}
        if recipe == "wm_two_valued":
            return {"mat": np.where(rng.random(n) < 0.5, np.float32(-3.5), np.float32(12.25)).astype(np.float32)}
        if recipe == "wm_occlusion":                        # an occlusion map of the default range: labels -15..0, sentinel -115
            mat = rng.integers(-15, 1, size=n).astype(np.float32)
            mat[rng.random(n) < 0.2] = -115.0
            return {"mat": mat}
        mat = (rng.standard_normal(n) * 100.0).astype(np.float32)
        if recipe == "wm_first_min":
            mat[0] = mat.min() - np.float32(40.0)
        elif recipe in ("wm_increasing", "wm_decreasing"):
            mat = np.unique(mat)                            # sorted, no two equal
            mat = np.ascontiguousarray(mat if recipe == "wm_increasing" else mat[::-1])
            assert mat.size == n
        else:
            assert recipe == "wm_random", recipe
        return {"mat": mat}
    assert mode == "gray"
    if recipe == "gray_lattice":                            # every (r, g, b) on a 5-step lattice, incl. sums that land on integers
        v = np.arange(0, 256, 5, dtype=np.uint8)
        return {"rgb": np.ascontiguousarray(np.stack(np.meshgrid(v, v, v, indexing="ij"), -1).reshape(1, -1, 3))}
    return {"rgb": rng.integers(0, 256, size=(h, w, c["channels"]), dtype=np.uint8)}


def driver_args(c):
    """Command line of oracle/ref_driver.cpp after the directory."""
    w, h = c["w"], c["h"]
    if c["mode"] == "pair":
        return [w, h, c.get("channels", 1)]
    if c["mode"] == "gf":
        return [w, h, c["size_d"], c["dmin"]]
    if c["mode"] == "occ":
        return [w, h, c["d_occlusion"], c["vmin"]]
    if c["mode"] == "wm":
        return [w * h]
    return [w * h, c["channels"]]


# fixture key -> (driver output file, dtype, is a volume)
OUTPUTS = {
    "pair": {"meanl": ("mean1.u8", np.uint8, False), "meanr": ("mean2.u8", np.uint8, False),
             "bestl": ("best_costl.f32", np.float32, False), "bestr": ("best_costr.f32", np.float32, False),
             "dmapl": ("dmapl.f32", np.float32, False), "dmapr": ("dmapr.f32", np.float32, False),
             "occlusion": ("occlusion.f32", np.float32, False), "filled": ("occlusion_filled.f32", np.float32, False),
             "grayl": ("I_l.u8", np.uint8, True), "grayr": ("I_r.u8", np.uint8, True),        # (hashed: they are inputs)
             "costl": ("costl.f32", np.float32, True), "costr": ("costr.f32", np.float32, True),
             "aggl": ("aggl.f32", np.float32, True), "aggr": ("aggr.f32", np.float32, True)},
    "gf": {"best": ("best_out.f32", np.float32, False), "dmap": ("dmap_out.f32", np.float32, False),
           "mean": ("mean.u8", np.uint8, False), "agg": ("agg.f32", np.float32, True)},
    "occ": {"occlusion": ("occlusion.f32", np.float32, False), "filled": ("filled.f32", np.float32, False)},
    "gray": {"gray": ("gray.u8", np.uint8, False)},
    "wm": {"u8": ("mat.u8", np.uint8, False)},
}


def sha256_canonical(a):
    """sha256 of the raw bytes, every f32 NaN first set to 0x7FC00000 (payload and sign are not part of the contract)."""
    import hashlib
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        u = a.view(np.uint32).copy()
        u[np.isnan(a)] = 0x7FC00000
        a = u
    return hashlib.sha256(a.tobytes()).hexdigest()
