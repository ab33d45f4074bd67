"""Deterministic draws for the fuzz of the opt-in stages (tests/test_gpu_optin_fuzz.py, tools/fuzz_optin.py): shapes, images,
disparity maps, cost volumes, parameters and the form of the call, all from np.random.default_rng(base + seed) and nothing
else -- no global state, so a case is named by (stage, base, seed).  A plain helper module, imported by name like the
*_ref.py files; tests/test_fuzz_scenes_cpu.py holds it to what the GPU tests rely on (every draw inside the contract of
include/smx.h, the regimes the kernels have to meet actually met), on the numpy references alone.

  shapes      half of the draws of a dimension come from the edge list k*T - 1, k*T, k*T + 1 of the stage's tile constants T,
              the other half are uniform in the range; D is then cut so that w*h*D stays below CELLS (a reference call
              stays far below two seconds and a test id in the seconds).
  images      kind = seed % 4: noise | 3..11 constant rectangles + noise of +-4 | the rectangles alone | one constant.
              A stereo pair is a wide image's columns [0, w) and [shift, shift + w).  A fourth channel is always noise.
  maps        rectangles scaled into [dmin, dmin + D), 15 % invalidated to dmin - 100, 5 % random valid labels, and on every
              third seed the messy values (NaN, +-inf, fractions, -0, the label behind the range, beyond int).
  volumes     kind = (seed // 4 + seed) % 4: integers 0..62 | integers 0..255 | floats in [0, 20) | special (negative, above
              SGM's clamp, NaN, +-inf, -0).
  call form   views both / left / right, any subset of agg, nbr, uq, a workspace for c of the slices in flight, a bound on
              the slices per launch, the slice range cut into 1..3 consecutive calls.
  compositions  one option set per seed (cost, aggregation, sub-pixel, uniqueness, speckle, weighted median, slices in
              flight) on one shape per base, with the numpy chain they have to equal (composition_reference).
  the table   a second family of compositions over EVERY row of the context's stage table (csrc/smx_ctx_plan.h): the walk
              TABLE_WALK pairs twelve aggregation families (guided, guided rgb, sgm, cross, scanline, cross-scanline, bp,
              patchmatch, and both guided ones under cross-scale and under the permeability filter) with the five costs
              (reference, census, AD-Census gray / colour, MI), one seed per pair the context accepts, through the gray or the
              rgb entry; behind the winners uniqueness, sub-pixel, speckle, vote, adjustment and the weighted median are drawn
              on top, and so are the call form and the order of the setters.  The pairs have depth steps (pair_steps).
              table_refusals states what a context refuses, from include/smx.h; table_reference is the numpy chain in the
              order of ctx_enqueue, with mi_ref.pair_loop around it under the MI cost.
"""
import numpy as np

import census_ref
import cross_ref

F32 = np.float32
# (appended to: BASE goes by position)
STAGES = ("census", "adcensus", "cgf", "cross", "sgm", "wta", "speckle", "wmf", "permeability", "bp", "mi", "patchmatch")
BASE = {s: 31000 + 1000 * i for i, s in enumerate(STAGES)}          # the committed seeds: BASE[stage] + 0 .. SEEDS - 1
SEEDS = 12
CELLS = 250_000                  # w * h * D of a drawn volume, at most
WINDOWS = [(1, 1), (4, 1), (2, 3), (4, 3)]          # (rx, ry): tests/test_gpu_census.py WINDOWS
KINDS = ("noise", "patches+noise", "patches", "constant")
VOLUMES = ("0..62", "0..255", "floats", "special")
SGM_D = (63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256)

# the tile constants of the kernels: (columns, rows, slices)
TILES = {
    "census": ((64, 256), (8,), (16,)),
    "adcensus": ((256,), (8,), (16,)),
    "cgf": ((32,), (64,), (8,)),
    "cross": ((64, 128, 192), (64, 128), (8,)),          # (rows: cross() takes the ring of 2 l1 + 2 rows of its drawn l1)
    "sgm": ((64,), (8,), (64,)),
    "wta": ((64,), (8, 64), (8,)),
    "speckle": ((64,), (16,), ()),
    "wmf": ((64,), (8,), ()),
    # smx_perm.hip: PW_PX, PH_COLS, PV_COLS columns; PH_ROWS rows of a wave, P_U rows a lane loads ahead; the slices go in chunks
    "permeability": ((8, 32, 256), (64, 8), ()),
    # smx_bp.hip: BP_WAVES sending pixels per workgroup, and the pyramid halves both axes per level (2, 4, 8 at levels 2 .. 4);
    # the labels go in waves of 64
    "bp": ((4, 8, 64), (2, 4, 8), (64,)),
    # smx_mi.hip: MI_COLS x MI_ROWS pixels a cost workgroup, MI_Z slices staged at a time (MI_THREADS pixels a histogram one)
    "mi": ((256,), (4,), (256,)),
    # smx_patchmatch.hip: PM_TW pixels of one colour a wave, so 2 PM_TW columns of a red-black pass; PM_TH rows a workgroup
    "patchmatch": ((64, 128), (4,), ()),
}


def rng_of(stage, seed, base=None):
    return np.random.default_rng((BASE[stage] if base is None else int(base)) + int(seed))


# ---------------------------------------------------------------------------------------------
# shapes
# ---------------------------------------------------------------------------------------------
def edge_list(tiles, lo, hi):
    return sorted({k * T + e for T in tiles for k in range(1, hi // T + 2) for e in (-1, 0, 1) if lo <= k * T + e <= hi})


def dim(rng, tiles, lo, hi):
    """one dimension in lo .. hi: from the edge list of `tiles` on half of the draws"""
    edges = edge_list(tiles, lo, hi)
    pick, uniform = rng.random() < 0.5, int(rng.integers(lo, hi + 1))          # (both drawn: one stream whatever the branch)
    return int(edges[int(rng.integers(0, len(edges)))]) if edges and pick else uniform


def shape(rng, stage, wmin=1, wmax=330, hmax=150, dmax=40, cells=CELLS):
    cols, rows, slices = TILES[stage]
    w, h = dim(rng, cols, wmin, wmax), dim(rng, rows, 1, hmax)
    D = dim(rng, slices, 1, dmax) if dmax > 1 else 1
    return w, h, max(1, min(D, cells // (w * h)))


# ---------------------------------------------------------------------------------------------
# images, maps, volumes
# ---------------------------------------------------------------------------------------------
def rectangles(rng, w, h, ch, lo, hi):
    """(h, w, ch) int64: a constant with 3 .. 11 constant rectangles on it, values in [lo, hi)"""
    img = np.empty((h, w, ch), np.int64)
    img[:] = rng.integers(lo, hi, ch)
    for _ in range(int(rng.integers(3, 12))):
        x0, x1 = sorted(int(t) for t in rng.integers(0, w + 1, 2))
        y0, y1 = sorted(int(t) for t in rng.integers(0, h + 1, 2))
        img[y0:y1, x0:x1] = rng.integers(lo, hi, ch)
    return img


def image(rng, kind, w, h, ch=1):
    """(h, w) uint8 for ch == 1, else (h, w, ch); a fourth channel is noise whatever the kind"""
    if kind == 0:
        img = rng.integers(0, 256, (h, w, ch))
    elif kind in (1, 2):
        img = rectangles(rng, w, h, ch, 4, 252)
        if kind == 1:
            img = img + rng.integers(-4, 5, (h, w, ch))
    else:
        img = np.empty((h, w, ch), np.int64)
        img[:] = rng.integers(0, 256, ch)
    img = img.astype(np.uint8)
    if ch == 4:
        img[:, :, 3] = rng.integers(0, 256, (h, w))
    return np.ascontiguousarray(img[:, :, 0] if ch == 1 else img)


def pair(rng, kind, w, h, D, ch=1):
    """left = columns [0, w) of a wide image, right = columns [shift, shift + w): the existing fuzz tests' pair"""
    shift = int(rng.integers(0, max(1, min(D, w // 3))))
    wide = image(rng, kind, w + D + 8, h, ch)
    return np.ascontiguousarray(wide[:, :w]), np.ascontiguousarray(wide[:, shift:shift + w])


def messy(rng, d, dmin, D):
    """the values of the stage tests' _messy helpers, and one beyond int, into 2 % of the pixels each"""
    m = rng.random(d.shape)
    d = d.copy()
    d[m < 0.02] = np.nan
    d[(m >= 0.02) & (m < 0.04)] = np.inf
    d[(m >= 0.04) & (m < 0.06)] = -np.inf
    d[(m >= 0.06) & (m < 0.08)] += F32(0.25)
    d[(m >= 0.08) & (m < 0.10)] = dmin + D
    d[(m >= 0.10) & (m < 0.12)] = -0.0
    d[(m >= 0.12) & (m < 0.13)] = 3e9
    d[(m >= 0.13) & (m < 0.14)] = -3e9
    return d


def disparity(rng, seed, w, h, dmin, D):
    """(h, w) float32 labels of [dmin, dmin + D) in rectangles, with the LR check's marker and outliers"""
    d = (dmin + rectangles(rng, w, h, 1, 0, D)[:, :, 0]).astype(F32)
    m = rng.random((h, w))
    other = (dmin + rng.integers(0, D, (h, w))).astype(F32)
    d[m < 0.15] = dmin - 100
    d = np.where((m >= 0.15) & (m < 0.20), other, d).astype(F32)
    return messy(rng, d, dmin, D) if seed % 3 == 0 else d


def volume(rng, kind, D, h, w):
    """(D, h, w) float32"""
    if kind == 0:
        return rng.integers(0, 63, (D, h, w)).astype(F32)
    if kind == 1:
        return rng.integers(0, 256, (D, h, w)).astype(F32)
    if kind == 2:
        return (rng.random((D, h, w)) * 20).astype(F32)
    c = (rng.random((D, h, w)) * 300 - 30).astype(F32)          # tests/test_gpu_cross.py _costs("special")
    flat = c.reshape(-1)
    idx = rng.permutation(flat.size)
    specials = np.array([np.nan, np.inf, -np.inf, -0.0, -1e30, 1e30, 255.0, 255.5, 256.0, 0.999], F32)
    for k, s in enumerate(specials):
        flat[idx[k::len(specials)][:max(1, flat.size // 40)]] = s
    return c


def volume_kind(seed):
    return (seed // 4 + seed) % 4


# ---------------------------------------------------------------------------------------------
# the form of a call
# ---------------------------------------------------------------------------------------------
def call_form(rng, count, outputs=("agg", "nbr", "uq")):
    """views, optional outputs, c = slices the workspace holds, the bound on the slices per launch, the consecutive ranges"""
    views = ("both", "both", "left", "right")[int(rng.integers(0, 4))]
    outs = {k: bool(rng.integers(0, 2)) for k in outputs}
    c = int(rng.integers(1, count + 1))
    bound = int(rng.choice([0, 1, 3, 7, 8, 9, count]))
    ncalls = int(rng.integers(1, min(3, count) + 1))
    cuts = sorted(int(t) for t in rng.choice(np.arange(1, count), ncalls - 1, replace=False)) if ncalls > 1 else []
    return dict(views=views, outs=outs, c=c, bound=bound, ranges=list(zip([0] + cuts, cuts + [count])))


def launches(form):
    """[(first slice, end)] of every launch of the drawn chunking: per call, chunks of min(c, bound or c) slices"""
    step = min(form["c"], form["bound"] or form["c"])
    return [(s, min(s1, s + step)) for s0, s1 in form["ranges"] for s in range(s0, s1, step)]


def form_text(form):
    outs = "+".join(k for k, on in form["outs"].items() if on) or "-"
    return f"{form['views']} outs {outs} c {form['c']} bound {form['bound']} calls {form['ranges']}"


def ranges_of(rng, D):
    """dminl in -(2 D + 3) .. 0, dminr in -3 .. D + 3: ranges wholly outside the image included"""
    return int(-rng.integers(0, 2 * D + 4)), int(rng.integers(-3, D + 4))


def sub_range(rng, D):
    """[s0, s1) of 0 .. D, any length: no multiple of 16, and empty on one draw in eight"""
    s0 = int(rng.integers(0, D + 1))
    s1 = s0 if rng.random() < 0.125 else int(rng.integers(s0, D + 1))
    return s0, s1


# ---------------------------------------------------------------------------------------------
# the stages: draw(stage, seed, base) -> dict with the arrays, the parameters (plain numbers) and "text"
# ---------------------------------------------------------------------------------------------
def census(seed, base=None):
    rng = rng_of("census", seed, base)
    w, h, D = shape(rng, "census")
    rx, ry = WINDOWS[int(rng.integers(0, len(WINDOWS)))]
    th = int(rng.integers(1, census_ref.nbits(rx, ry) + 1))
    dminl, dminr = ranges_of(rng, D)
    s0, s1 = sub_range(rng, D)
    views = ("both", "both", "left", "right")[int(rng.integers(0, 4))]
    per_launch = int(rng.integers(1, 3))                  # images per smx_dev_census launch
    Il, Ir = pair(rng, seed % 4, w, h, D)
    return dict(w=w, h=h, D=D, rx=rx, ry=ry, th=th, dminl=dminl, dminr=dminr, s0=s0, s1=s1, views=views, per_launch=per_launch,
                Il=Il, Ir=Ir, text=f"{w}x{h}x{D} {KINDS[seed % 4]} window {rx},{ry} th {th} dmin {dminl},{dminr} "
                                   f"slices [{s0},{s1}) {views} {per_launch} image(s) per launch")


def adcensus(seed, base=None):
    rng = rng_of("adcensus", seed, base)
    w, h, D = shape(rng, "adcensus")
    rx, ry = WINDOWS[int(rng.integers(0, len(WINDOWS)))]
    th = int(rng.integers(1, census_ref.nbits(rx, ry) + 1))
    ch = int(rng.choice([1, 3, 4]))
    colour = int(ch > 1)
    lc = float(rng.choice([30.0, 10.0, 45.5, 1.0]))
    la = float(rng.choice([10.0, 5.0, 20.25, 0.5]))
    scale = float(rng.choice([127.5, 100.0, 1.0, 255.0]))
    dminl, dminr = ranges_of(rng, D)
    s0, s1 = sub_range(rng, D)
    views = ("both", "both", "left", "right")[int(rng.integers(0, 4))]
    gl, gr = pair(rng, seed % 4, w, h, D)
    imgs = pair(rng, seed % 4, w, h, D, ch) if colour else (gl, gr)
    return dict(w=w, h=h, D=D, rx=rx, ry=ry, th=th, ch=ch, colour=colour, lambda_census=lc, lambda_ad=la, scale=scale, dminl=dminl,
                dminr=dminr, s0=s0, s1=s1, views=views, grays=(gl, gr), imgs=imgs,
                text=f"{w}x{h}x{D} {KINDS[seed % 4]} ch {ch} window {rx},{ry} th {th} lambda {lc},{la} scale {scale} "
                     f"dmin {dminl},{dminr} slices [{s0},{s1}) {views}")


def _aggregation(rng, stage, seed, guide_ch, kinds=4, **kw):
    """shape, the guides and cost volumes of both views, the call form"""
    w, h, D = shape(rng, stage, **kw)
    ch = int(rng.choice(guide_ch))
    kind = volume_kind(seed) % kinds
    gl, gr = pair(rng, seed % 4, w, h, D, ch)
    if ch == 1:
        gl, gr = gl[:, :, None], gr[:, :, None]
    costs = (volume(rng, kind, D, h, w), volume(rng, kind, D, h, w))
    return dict(w=w, h=h, D=D, ch=ch, guides=(gl, gr), costs=costs, form=call_form(rng, D)), f"{w}x{h}x{D} {KINDS[seed % 4]} " \
        f"ch {ch} costs {VOLUMES[kind]}"


def cgf(seed, base=None):
    rng = rng_of("cgf", seed, base)
    case, text = _aggregation(rng, "cgf", seed, [3, 4], cells=120_000)
    case.update(radius=int(rng.integers(0, 13)), eps=float(rng.choice([0.01, 0.5, 6.5025, 100.0])))
    case["text"] = f"{text} radius {case['radius']} eps {case['eps']} {form_text(case['form'])}"
    return case


def cross(seed, base=None):
    rng = rng_of("cross", seed, base)
    l1 = 63 if rng.random() < 0.35 else int(rng.integers(1, 64))
    l2 = int(rng.integers(0, l1 + 1))
    tau1 = int(rng.choice([6, 12, 20, 40, 256]))
    tau2 = int(rng.integers(1, tau1 + 1)) if rng.random() < 0.7 else tau1
    iterations = int(rng.integers(1, 5))
    cols, _, slices = TILES["cross"]
    rows = tuple(sorted({2 * l1 + 2, l1, 64}))            # h on both sides of the ring of 2 l1 + 2 rows, and around l1
    w, h = dim(rng, cols, 1, 330), dim(rng, rows, 1, 150)
    h = max(1, min(h, 16_000 // w))                       # (the reference's arms cost l1 passes over the image per direction)
    D = max(1, min(dim(rng, slices, 1, 40), 100_000 // (w * h)))
    ch = int(rng.choice([1, 3, 4]))
    kind = volume_kind(seed)
    gl, gr = pair(rng, seed % 4, w, h, D, ch)
    if ch == 1:
        gl, gr = gl[:, :, None], gr[:, :, None]
    costs = (volume(rng, kind, D, h, w), volume(rng, kind, D, h, w))
    form = call_form(rng, D)
    return dict(w=w, h=h, D=D, ch=ch, guides=(gl, gr), costs=costs, form=form, l1=l1, l2=l2, tau1=tau1, tau2=tau2,
                iterations=iterations,
                text=f"{w}x{h}x{D} {KINDS[seed % 4]} ch {ch} costs {VOLUMES[kind]} l {l1},{l2} tau {tau1},{tau2} "
                     f"iterations {iterations} {form_text(form)}")


def sgm(seed, base=None):
    rng = rng_of("sgm", seed, base)
    if seed % 2:                                      # the padded D of 64 / 128 / 192 / 256 on a small image
        D = int(rng.choice(SGM_D))
        w = int(rng.integers(1, 100))
        h = int(rng.integers(1, max(2, 500 // w + 1)))
    else:
        w, h, D = shape(rng, "sgm", dmax=70, cells=150_000)
    p2 = int(rng.choice([0, 7, 120, 4095, int(rng.integers(0, 4096))]))
    p1 = int(rng.choice([0, p2, int(rng.integers(0, p2 + 1))]))
    paths = int(rng.choice([4, 8]))
    kind = volume_kind(seed)
    costs = (volume(rng, kind, D, h, w), volume(rng, kind, D, h, w))
    views = ("both", "both", "left", "right")[int(rng.integers(0, 4))]
    outs = {k: bool(rng.integers(0, 2)) for k in ("agg", "nbr", "uq")}
    on = "+".join(k for k, v in outs.items() if v) or "-"
    return dict(w=w, h=h, D=D, p1=p1, p2=p2, paths=paths, costs=costs, views=views, outs=outs,
                text=f"{w}x{h}x{D} costs {VOLUMES[kind]} p {p1},{p2} paths {paths} {views} outs {on}")


def wta(seed, base=None):
    """The guided-filter aggregation's _nbr / _uq entries on the paths 5 (comb walker), 3 (ring walker), 1 (multi-kernel)."""
    rng = rng_of("wta", seed, base)
    w, h, D = shape(rng, "wta", wmin=2, wmax=260, hmax=120, dmax=24, cells=200_000)
    path = (5, 3, 1)[seed % 3]
    radius = 9 if path == 5 else int(rng.integers(0, 10 if path == 3 else 13))
    params = dict(radius=radius, alpha=float(rng.choice([0.9, 0.5, 0.1])), th_color=int(rng.integers(1, 30)),
                  th_grad=int(rng.integers(1, 8)), eps=float(rng.choice([6.5025, 100.0, 1.0 if path == 5 else 0.5])),          # (the comb walker: eps >= 1)
                  d_lr=int(rng.integers(0, 3)))
    dminl, dminr = ranges_of(rng, D)
    Il, Ir = pair(rng, seed % 4, w, h, D)
    form = call_form(rng, D, outputs=("agg", "nbr", "mean"))
    form["views"] = "both"                            # (the _uq entry is a pair entry)
    fresh = bool(rng.integers(0, 2))
    ratio = float(rng.choice([0.05, 0.15, 0.25, 1.0]))
    return dict(w=w, h=h, D=D, path=path, params=params, dminl=dminl, dminr=dminr, Il=Il, Ir=Ir, form=form, fresh=fresh, ratio=ratio,
                text=f"{w}x{h}x{D} {KINDS[seed % 4]} path {path} radius {radius} alpha {params['alpha']} th {params['th_color']},"
                     f"{params['th_grad']} eps {params['eps']} d_lr {params['d_lr']} dmin {dminl},{dminr} fresh {int(fresh)} "
                     f"ratio {ratio} {form_text(form)}")


def speckle(seed, base=None):
    rng = rng_of("speckle", seed, base)
    w, h, _ = shape(rng, "speckle", dmax=1)
    D = int(rng.integers(1, 41))
    dmin = int(-rng.integers(0, 2 * D + 4))
    max_size = int(rng.choice([0, 1, 5, 30, 200, 100000]))
    max_diff = float(rng.choice([0.0, 1.0, 2.5]))
    in_place = bool(rng.integers(0, 2))
    d = disparity(rng, seed, w, h, dmin, D)
    return dict(w=w, h=h, D=D, dmin=dmin, max_size=max_size, max_diff=max_diff, in_place=in_place, disp=d,
                text=f"{w}x{h} labels [{dmin},{dmin + D}) max_size {max_size} max_diff {max_diff} "
                     f"{'in place' if in_place else 'out of place'}{' messy' if seed % 3 == 0 else ''}")


def wmf(seed, base=None):
    rng = rng_of("wmf", seed, base)
    if seed % 4 == 3:                                 # more than one bucket on the second histogram level, on a small map
        w, h = int(rng.integers(1, 60)), int(rng.integers(1, 40))
        D = int(rng.integers(65, 301))
    else:
        w, h, _ = shape(rng, "wmf", wmax=200, hmax=100, dmax=1)
        D = int(rng.integers(1, 65))
    dmin = int(-rng.integers(0, 2 * D + 4))
    radius = int(rng.integers(1, 16))                 # (smx_wmf_params: 1 <= radius <= 15)
    sigma_s = float(rng.choice([9.0, 1.5, 0.4, 1e9]))
    sigma_c = float(rng.choice([25.5, 4.0, 0.3, 1e9]))
    mode = ("occluded", "all")[int(rng.integers(0, 2))]
    guide = image(rng, seed % 4, w, h)
    d = disparity(rng, seed, w, h, dmin, D)
    # the selection of "occluded": the map's own markers, as a pair's occlusion map has them, and none in whole rectangles
    sel = np.where(rectangles(rng, w, h, 1, 0, 3)[:, :, 0] == 0, F32(dmin), d).astype(F32)
    return dict(w=w, h=h, D=D, dmin=dmin, radius=radius, sigma_s=sigma_s, sigma_c=sigma_c, mode=mode, guide=guide, disp=d,
                select=sel if mode == "occluded" else None,
                text=f"{w}x{h} labels [{dmin},{dmin + D}) {KINDS[seed % 4]} radius {radius} sigma {sigma_s},{sigma_c} {mode}"
                     f"{' messy' if seed % 3 == 0 else ''}")


PERM_STORES = ("none", "separate", "in place")          # tests/test_gpu_perm.py FORMS


def permeability(seed, base=None):
    """smx_dev_permeability_wta_pair: every form of tests/test_gpu_perm.py FORMS (views, the filtered volumes nowhere / apart / in
    place, the states) with a workspace for c of the slices and the calling thread's bound on the slices per launch"""
    rng = rng_of("permeability", seed, base)
    w, h, D = shape(rng, "permeability", dmax=24)
    ch = int(rng.choice([1, 3, 4]))
    sigma = float(rng.choice([32.0, 4.0, 0.011, 200.0, 1e6]))
    kind = volume_kind(seed)
    gl, gr = pair(rng, seed % 4, w, h, D, ch)
    costs = (volume(rng, kind, D, h, w), volume(rng, kind, D, h, w))
    views = ("both", "both", "left", "right")[int(rng.integers(0, 4))]
    store = PERM_STORES[int(rng.integers(0, 3))]
    nbr, uq = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
    c = int(rng.integers(1, D + 1)) if rng.random() < 0.6 else None          # (None: a workspace for every slice at once)
    bound = int(rng.choice([0, 0, 1, 3, 8, D]))
    return dict(w=w, h=h, D=D, ch=ch, sigma=sigma, guides=(gl, gr), costs=costs, views=views, store=store, nbr=nbr, uq=uq, c=c,
                bound=bound, text=f"{w}x{h}x{D} {KINDS[seed % 4]} ch {ch} costs {VOLUMES[kind]} sigma {sigma} {views} out {store} "
                                  f"nbr {int(nbr)} uq {int(uq)} c {c} bound {bound}")


def bp(seed, base=None):
    """smx_dev_bp_wta_pair: both views or one, any subset of agg / nbr / uq, a misaligned workspace"""
    rng = rng_of("bp", seed, base)
    if seed % 2:                                      # the padded D of 64 / 128 / 192 / 256 on a small image
        D = int(rng.choice(SGM_D))
        w = int(rng.integers(1, 100))
        h = int(rng.integers(1, max(2, 500 // w + 1)))
    else:
        w, h, D = shape(rng, "bp", wmax=200, hmax=100, dmax=70, cells=150_000)
    step, trunc = BP_PENALTIES[int(rng.integers(0, len(BP_PENALTIES)))]
    iterations, levels = int(rng.integers(0, 6)), int(rng.integers(1, 5))
    data_scale = float(rng.choice([1.0, 16.0, 0.5]))
    kind = volume_kind(seed)
    costs = (volume(rng, kind, D, h, w), volume(rng, kind, D, h, w))
    views = ("both", "both", "left", "right")[int(rng.integers(0, 4))]
    outs = {k: bool(rng.integers(0, 2)) for k in ("agg", "nbr", "uq")}
    misalign = int(rng.choice([0, 1, 13, 255]))
    on = "+".join(k for k, v in outs.items() if v) or "-"
    return dict(w=w, h=h, D=D, step=step, trunc=trunc, iterations=iterations, levels=levels, data_scale=data_scale, costs=costs,
                views=views, outs=outs, misalign=misalign,
                text=f"{w}x{h}x{D} costs {VOLUMES[kind]} V {step},{trunc} iterations {iterations} levels {levels} "
                     f"scale {data_scale} "
                     f"{views} outs {on} ws misaligned by {misalign}")


MI_D = (255, 256, 257, 300)          # around MI_Z
MI_TABLES = ("learned", "asymmetric")


def mi(seed, base=None):
    """smx_dev_mi_histogram, smx_dev_mi_table, smx_dev_mi_random_map and smx_dev_mi_cost_pair: a map with a third of its pixels
    marked and labels that send partners off both edges, the table learned from it or a random asymmetric one, a slice
    sub-range, both views or one"""
    rng = rng_of("mi", seed, base)
    if seed % 2:                                      # more slices than one staged span, on a small image
        D = int(rng.choice(MI_D))
        w = int(rng.integers(1, 100))
        h = int(rng.integers(1, max(2, 500 // w + 1)))
    else:
        w, h, D = shape(rng, "mi", hmax=100, dmax=70)
    dminl, dminr = ranges_of(rng, D)
    s0, s1 = sub_range(rng, D)
    views = ("both", "both", "left", "right")[int(rng.integers(0, 4))]
    table = MI_TABLES[int(rng.integers(0, 2))]
    Il, Ir = pair(rng, seed % 4, w, h, D)
    mark = dminl - 100
    disp = (dminl + rectangles(rng, w, h, 1, 0, D)[:, :, 0]).astype(F32)
    m = rng.random((h, w))
    disp = np.where(m < 0.1, rng.integers(-w - 2, w + 3, (h, w)).astype(F32), disp).astype(F32)
    disp[m > 2.0 / 3.0] = mark
    asym = rng.integers(0, 256, (256, 256)).astype(np.uint8)
    return dict(w=w, h=h, D=D, dminl=dminl, dminr=dminr, s0=s0, s1=s1, views=views, table=table, Il=Il, Ir=Ir, disp=disp,
                mark=mark, asym=asym, map_seed=int(rng.integers(0, 2 ** 32)),
                text=f"{w}x{h}x{D} {KINDS[seed % 4]} dmin {dminl},{dminr} slices [{s0},{s1}) {views} table {table}")


PM_ENTRIES = ("search", "search", "plane cost")
PM_WORK = 250_000          # pixels x window taps x iterations of a drawn search: its reference stays below a second


def patchmatch(seed, base=None):
    """smx_dev_patchmatch_pair (all four outputs) or smx_dev_pm_plane_cost (the cost of given planes alone, some of them outside
    the labels or not numbers), with the workspace misaligned"""
    rng = rng_of("patchmatch", seed, base)
    radius = int(rng.integers(0, 4))
    iterations = int(rng.integers(1, 3))
    w = dim(rng, TILES["patchmatch"][0], 1, 200)
    h = max(1, min(dim(rng, TILES["patchmatch"][1], 1, 40), PM_WORK // ((2 * radius + 1) ** 2 * iterations * w)))
    D = int(rng.integers(1, 41))
    dminl, dminr = ranges_of(rng, D)
    pm = dict(radius=radius, gamma=float(rng.choice([10.0, 1.0, 50.0])), iterations=iterations,
              max_slope=float(rng.choice([0.0, 2.0, 8.0])), seed=int(rng.integers(0, 2 ** 32)))
    entry = PM_ENTRIES[int(rng.integers(0, len(PM_ENTRIES)))]
    misalign = int(rng.choice([0, 1, 255]))
    left, right = pair(rng, seed % 4, w, h, D)
    planes = np.empty((2, 3, h, w), F32)
    planes[:, :2] = rng.uniform(-2.5, 2.5, (2, 2, h, w))
    planes[0, 2] = rng.uniform(dminl - 1.5, dminl + D + 0.5, (h, w))
    planes[1, 2] = rng.uniform(dminr - 1.5, dminr + D + 0.5, (h, w))
    flat = planes.reshape(-1)
    flat[rng.integers(0, flat.size, 4)] = np.array([np.nan, np.inf, -np.inf, 3e38], F32)
    return dict(w=w, h=h, D=D, dminl=dminl, dminr=dminr, pm=pm, entry=entry, misalign=misalign, left=left, right=right,
                planes=planes,
                text=f"{w}x{h}x{D} {KINDS[seed % 4]} dmin {dminl},{dminr} {entry} radius {radius} gamma {pm['gamma']} "
                     f"iterations {iterations} max_slope {pm['max_slope']} ws misaligned by {misalign}")


DRAW = dict(census=census, adcensus=adcensus, cgf=cgf, cross=cross, sgm=sgm, wta=wta, speckle=speckle, wmf=wmf,
            permeability=permeability, bp=bp, mi=mi, patchmatch=patchmatch)


# ---------------------------------------------------------------------------------------------
# compositions: one option set per seed, for both front ends (PairPipeline, smx_ctx) on ONE shape per base
# ---------------------------------------------------------------------------------------------
COMP_BASE = 41000
COSTS = ("reference", "census", "adcensus", "adcensus colour")
AGGS = ("guided", "guided rgb", "sgm", "cross", "cross rgb")


def composition_ok(cost, agg):
    """What the front ends refuse: cross-based aggregation takes the colour pair as its guide wherever one is given, and the
    colour AD term needs one -- so there is no gray cross with the colour cost.  (Colour guidance with SGM or cross is no
    member of AGGS; uniqueness comes without a slice sub-range here.)"""
    return not (cost == "adcensus colour" and agg == "cross")


def composition_setup(base=None):
    """the shape and the smx_params of a base's context: it lives across the seeds"""
    rng = np.random.default_rng(COMP_BASE if base is None else int(base))
    w, h = dim(rng, (64,), 40, 160), dim(rng, (8, 64), 24, 90)
    D = int(rng.integers(6, 20))
    return dict(w=w, h=h, D=D, radius=int(rng.integers(0, 13)), eps=float(rng.choice([6.5025, 100.0, 1.0])))


def composition(seed, base=None):
    s = composition_setup(base)
    w, h, D = s["w"], s["h"], s["D"]
    rng = np.random.default_rng((COMP_BASE if base is None else int(base)) + 1 + int(seed))
    cost, agg = COSTS[seed % 4], AGGS[(seed + 2 * (seed // 4)) % 5]
    if not composition_ok(cost, agg):
        agg = "cross rgb"
    rx, ry = WINDOWS[int(rng.integers(0, len(WINDOWS)))]
    l1 = int(rng.integers(1, 21))
    tau1 = int(rng.choice([12, 20, 40]))
    p2 = int(rng.choice([7, 120, 400]))
    opt = dict(cost=cost, agg=agg,
               census=dict(rx=rx, ry=ry, th=int(rng.integers(1, census_ref.nbits(rx, ry) + 1))),
               adcensus=dict(lambda_census=float(rng.choice([30.0, 10.0])), lambda_ad=float(rng.choice([10.0, 20.25])), scale=127.5),
               sgm=dict(p1=int(rng.integers(0, p2 + 1)), p2=p2, paths=int(rng.choice([4, 8]))),
               cross=dict(l1=l1, l2=int(rng.integers(0, l1 + 1)), tau1=tau1, tau2=int(rng.integers(1, tau1 + 1)),
                          iterations=int(rng.integers(1, 5))),
               subpixel=(None, "parabola", "equiangular")[int(rng.integers(0, 3))],
               uniqueness=(None, 5, 15, 40)[int(rng.integers(0, 4))],                  # OpenCV's percent: ratio = u / (100 - u)
               speckle=None if rng.random() < 0.4 else (int(rng.choice([5, 30, 200])), float(rng.choice([0.0, 1.0, 2.5]))),
               wmf=(None, "occluded", "all")[int(rng.integers(0, 3))],
               sif=int(rng.integers(1, D + 1)), bound=int(rng.choice([0, 1, 3, 7, 8, 9, D])), volumes=bool(rng.integers(0, 2)))
    dminl, dminr = int(-rng.integers(0, D + 3)), int(rng.integers(-3, 4))
    ch = int(rng.choice([3, 4]))
    rgb = pair(rng, (1, 2, 0, 1)[seed % 4], w, h, D, ch)              # (mostly structured: the later stages need surfaces)
    on = " ".join(f"{k} {opt[k]}" for k in ("subpixel", "uniqueness", "speckle", "wmf"))
    return dict(s, opt=opt, dminl=dminl, dminr=dminr, ch=ch, rgb=rgb,
                text=f"{w}x{h}x{D} ch {ch} radius {s['radius']} eps {s['eps']} cost {cost} agg {agg} {on} dmin {dminl},{dminr} "
                     f"sif {opt['sif']} bound {opt['bound']} volumes {int(opt['volumes'])}")


def composition_reference(c, orc):
    """The numpy chain of a drawn composition: the stage references, the oracle for the reference's own stages, and
    main_harness.finish_chain behind the winners.  -> dict named like PairPipeline.results()."""
    import ctypes
    import adcensus_ref
    import cgf_ref
    import main_harness
    import sgm_ref
    import subpix_ref
    o, D = c["opt"], c["D"]
    P = orc.Params()
    orc.lib().orc_default_params(ctypes.byref(P))
    P.radius, P.eps = c["radius"], c["eps"]
    rgb = c["rgb"]
    gray = [orc.gray(i, params=P) for i in rgb]
    dmin = (c["dminl"], c["dminr"])
    cost = []
    for v in (0, 1):
        if o["cost"] == "reference":
            cost.append(orc.cost_volume(gray[v], gray[1 - v], D, dmin[v], params=P))
        elif o["cost"] == "census":
            cost.append(census_ref.census_cost(gray[v], gray[1 - v], D, dmin[v], **o["census"]))
        else:
            colour = int(o["cost"] == "adcensus colour")
            img = rgb if colour else gray
            cost.append(adcensus_ref.cost(img[v], img[1 - v], gray[v], gray[1 - v], D, dmin[v], colour=colour, **o["census"],
                                          **o["adcensus"]))
    q = []
    with np.errstate(all="ignore"):
        for v in (0, 1):
            if o["agg"] == "guided":
                q.append(orc.guided_filter(gray[v], cost[v], dmin[v], want_agg=True, params=P)[3])
            elif o["agg"] == "guided rgb":
                q.append(cgf_ref.aggregate(rgb[v], cost[v], c["radius"], c["eps"]))
            elif o["agg"] == "sgm":
                q.append(sgm_ref.aggregate(cost[v], **o["sgm"]).astype(F32))
            else:
                guide = rgb[v] if o["agg"] == "cross rgb" else gray[v]
                q.append(cross_ref.aggregate(guide, cost[v], **o["cross"]))
    st = [cgf_ref.states(v) for v in q]
    assert all((s["z"] >= 0).all() for s in st)
    e = dict(aggl=q[0], aggr=q[1], costl=cost[0], costr=cost[1], grayl=gray[0], grayr=gray[1], bestl=st[0]["best"], bestr=st[1]["best"],
             dmapl=subpix_ref.dmap_of(st[0]["z"], st[0]["best"], dmin[0]), dmapr=subpix_ref.dmap_of(st[1]["z"], st[1]["best"], dmin[1]),
             keys=np.stack([s["keys"] for s in st]))
    main_harness.finish_chain(orc, e, c["dminl"], D, z=st[0]["z"], best=st[0]["best"], sec=st[0]["uq"][0], nbr=st[0]["nbr"],
                              uniqueness=o["uniqueness"], speckle=o["speckle"], subpixel=o["subpixel"], wmf=o["wmf"])
    if o["subpixel"]:
        mode = subpix_ref.MODES[o["subpixel"]]
        for v, k in enumerate(("subpixl", "subpixr")):
            e[k], _ = subpix_ref.maps(mode, st[v]["z"], st[v]["best"], st[v]["nbr"][0], st[v]["nbr"][1], e["dmap" + "lr"[v]])
        e["subpix_filled"] = e["sub_filled"]
    return e


def ratio_of(percent):
    """the ratio of OpenCV's uniquenessRatio percent, in float32 as main_harness.finish_chain takes it"""
    return float(F32(percent) / (F32(100.0) - F32(percent)))


# ---------------------------------------------------------------------------------------------
# the table family: one option set per seed over EVERY row of the context's stage table, on one shape per base
# ---------------------------------------------------------------------------------------------
TABLE_BASE = 43200
TABLE_COSTS = ("reference", "census", "adcensus", "adcensus colour", "mi")
# family -> (the aggregation, colour guidance, what runs over the guided filter's volumes)
FAMILIES = {
    "guided": ("guided", False, None), "guided+cross_scale": ("guided", False, "cross_scale"),
    "guided rgb": ("guided", True, None), "guided rgb+cross_scale": ("guided", True, "cross_scale"),
    "sgm": ("sgm", False, None), "cross": ("cross", False, None), "guided+permeability": ("guided", False, "permeability"),
    "scanline": ("scanline", False, None), "guided rgb+permeability": ("guided", True, "permeability"),
    "cross-scanline": ("cross-scanline", False, None), "bp": ("bp", False, None), "patchmatch": ("patchmatch", False, None),
}
TABLE_FAMILIES = tuple(FAMILIES)
BP_PENALTIES = [(20, 60), (0, 0), (7, 7), (1, 4095), (4095, 4095)]          # tests/test_gpu_bp.py PENALTIES
PM_GAMMA = 10.0                                                             # smx_default_pm_params

# What include/smx.h says does not run together, by the names of a context's settings (the setters' paragraphs; the C++ table
# of csrc/smx_ctx_plan.h is not read here: tests/test_fuzz_scenes_cpu.py holds this to tests/ctx_plan_ref.py).
TABLE_REPLACING = ("sgm", "cross", "so", "bp", "pm")          # they take the place of the guided filter ...
TABLE_GUIDED_ONLY = ("cgf", "cscale", "perm")                 # ... and these belong to it
TABLE_EXCLUDES = tuple(
    [(a, b) for i, a in enumerate(TABLE_REPLACING) for b in TABLE_REPLACING[i + 1:] if (a, b) != ("cross", "so")] +
    [(a, b) for a in TABLE_REPLACING for b in TABLE_GUIDED_ONLY] + [("cscale", "perm")] +
    [("pm", b) for b in ("census", "adcensus", "adjust", "uniq", "subpix")])          # (the MI cost is a mode of "census")
TABLE_MAX_D = {"sgm": 256, "so": 256, "bp": 256, "adjust": 512, "vote": 512}


def table_walk():
    """[(family, cost, entry, volumes)] in seed order: every pair of an aggregation family and a cost that a context accepts, once;
    PatchMatch takes the reference's cost only and comes once per entry.  The entry is "rgb" where the settings need the colour
    pair (colour guidance, the colour AD term), else it alternates over the walk, so that both occur under every family; so
    does `volumes`, at half
    the rate (PatchMatch stereo has no volumes to hand out)."""
    out = []
    for f, fam in enumerate(TABLE_FAMILIES):
        for k, cost in enumerate(TABLE_COSTS):
            if fam == "patchmatch" and cost != "reference":
                continue
            forced = FAMILIES[fam][1] or cost == "adcensus colour"
            out.append((fam, cost, "rgb" if forced or (f + k) % 2 else "gray", fam != "patchmatch" and bool((f + k) // 2 % 2)))
    out.append(("patchmatch", "reference", "gray" if out[-1][2] == "rgb" else "rgb", False))
    return tuple(out)


TABLE_WALK = table_walk()
# the setters of a context, each called for every case in the order the case draws ("order": indices into this)
TABLE_SETTERS = ("cost", "adcensus", "mi", "aggregation", "guidance", "cross", "scanline", "bp", "patchmatch", "cross_scale",
                 "permeability", "subpixel", "uniqueness", "speckle", "vote", "adjust")
TABLE_SEEDS = len(TABLE_WALK)          # 57: the committed seeds of the table family are TABLE_BASE + 1 + 0 .. TABLE_SEEDS - 1


def pair_steps(rng, kind, w, h, D, ch=1):
    """pair() with 1 .. 3 rectangles of the right view taken at shifts of their own: depth steps and the occlusions beside
    them, which the LR check, the vote and the adjustment need (a pair that is one shift has one depth)"""
    smax = max(1, min(D, w // 3))
    shift = int(rng.integers(0, smax))
    wide = image(rng, kind, w + D + 8, h, ch)
    left, right = wide[:, :w].copy(), wide[:, shift:shift + w].copy()
    for _ in range(int(rng.integers(1, 4))):
        x0, x1 = sorted(int(t) for t in rng.integers(0, w + 1, 2))
        y0, y1 = sorted(int(t) for t in rng.integers(0, h + 1, 2))
        s = int(rng.integers(0, smax))
        right[y0:y1, x0:x1] = wide[y0:y1, x0 + s:x1 + s]
    return np.ascontiguousarray(left), np.ascontiguousarray(right)


def table_setup(base=None):
    """the shape and the smx_params of a base's context (and of its cross-scale children): they live across the seeds.  At most
    9100 pixels: the PatchMatch reference at radius 2 and 2 iterations stays below two seconds."""
    rng = np.random.default_rng(TABLE_BASE if base is None else int(base))
    while True:
        w, h = dim(rng, (64,), 40, 130), dim(rng, (8, 64), 24, 70)
        if w * h <= 9100:
            break
    D = int(rng.integers(6, 21))
    return dict(w=w, h=h, D=D, radius=int(rng.integers(0, 13)), eps=float(rng.choice([6.5025, 100.0, 1.0])))


def table_settings(c):
    """the settings of a drawn case by the names of tests/ctx_plan_ref.py (SETTERS and "adc_colour"; the MI cost is a mode of
    the census cost's row)"""
    o = c["opt"]
    agg, cgf, extra = FAMILIES[o["family"]]
    return dict(census=o["cost"] in ("census", "mi"), adcensus=o["cost"].startswith("adcensus"),
                adc_colour=o["cost"] == "adcensus colour",
                sgm=agg == "sgm", cgf=cgf, cross=agg in ("cross", "cross-scanline"), so=agg in ("scanline", "cross-scanline"),
                cscale=extra == "cross_scale", perm=extra == "permeability", bp=agg == "bp", pm=agg == "patchmatch",
                adjust=bool(o["adjust"]), uniq=bool(o["uniqueness"]), subpix=bool(o["subpixel"]), speckle=bool(o["speckle"]),
                vote=bool(o["vote"]))


def table_excluded(s):
    """the pairs of TABLE_EXCLUDES that the settings `s` (table_settings) have on together"""
    return [f"{a} with {b}" for a, b in TABLE_EXCLUDES if s[a] and s[b]]


def table_refusals(c):
    """why a context would refuse the drawn case (empty: it takes it), from TABLE_EXCLUDES and the limits of include/smx.h"""
    s, o = table_settings(c), c["opt"]
    why = table_excluded(s)
    if s["pm"] and o["volumes"]:
        why.append("PatchMatch stereo produces no volumes")
    if (s["cgf"] or s["adc_colour"]) and c["entry"] != "rgb":
        why.append("the colour pair comes through the rgb entry")
    why += [f"{k} takes at most {m} labels" for k, m in TABLE_MAX_D.items() if s[k] and c["D"] > m]
    if s["cscale"] and (c["w"] + (1 << (o["cross_scale"]["scales"] - 1)) - 1) >> (o["cross_scale"]["scales"] - 1) < 2:
        why.append("the coarsest cross-scale level is narrower than 2 pixels")
    return why


def _table_options(rng, s, fam, cost, volumes, mi_init):
    """one option set behind the walk's (family, cost, entry): every stage's parameters are drawn whether the stage is on or
    not, so that the stream does not depend on the walk"""
    D = s["D"]
    rx, ry = WINDOWS[int(rng.integers(0, len(WINDOWS)))]
    l1 = int(rng.integers(1, 21))
    tau1 = int(rng.choice([12, 20, 40]))
    p2 = int(rng.choice([7, 120, 400]))
    so_p2 = int(rng.choice([7, 382, 4095]))
    step, trunc = BP_PENALTIES[int(rng.integers(0, len(BP_PENALTIES)))]
    vl1 = int(rng.integers(1, 21))
    vtau1 = int(rng.choice([12, 20, 40]))
    opt = dict(
        family=fam, cost=cost,
        census=dict(rx=rx, ry=ry, th=int(rng.integers(1, census_ref.nbits(rx, ry) + 1))),
        adcensus=dict(lambda_census=float(rng.choice([30.0, 10.0])), lambda_ad=float(rng.choice([10.0, 20.25])), scale=127.5),
        mi=dict(iterations=int(rng.integers(1, 3)), init=mi_init, seed=int(rng.integers(0, 2 ** 32))),
        sgm=dict(p1=int(rng.integers(0, p2 + 1)), p2=p2, paths=int(rng.choice([4, 8]))),
        cross=dict(l1=l1, l2=int(rng.integers(0, l1 + 1)), tau1=tau1, tau2=int(rng.integers(1, tau1 + 1)),
                   iterations=int(rng.integers(1, 5))),
        scanline=dict(p1=int(rng.integers(0, so_p2 + 1)), p2=so_p2, tau_so=int(rng.choice([1, 15, 256])),
                      paths=int(rng.choice([4, 8]))),
        bp=dict(step=step, trunc=trunc, iterations=int(rng.integers(1, 6)), levels=int(rng.integers(1, 5)),
                data_scale=float(rng.choice([1.0, 16.0]))),
        patchmatch=dict(radius=int(rng.integers(0, 3)), gamma=PM_GAMMA, iterations=int(rng.integers(1, 3)),
                        max_slope=float(rng.choice([0.0, 2.0])), seed=int(rng.integers(0, 2 ** 32))),
        cross_scale=dict(scales=int(rng.integers(1, 5)), lambda_=float(rng.choice([0.0, 0.3, 1.0]))),
        permeability=dict(sigma=float(rng.choice([4.0, 32.0, 1e6]))),
        subpixel=(None, "parabola", "equiangular")[int(rng.integers(0, 3))],
        uniqueness=(None, 5, 15, 40)[int(rng.integers(0, 4))],
        speckle=None if rng.random() < 0.4 else (int(rng.choice([5, 30, 200])), float(rng.choice([0.0, 1.0, 2.5]))),
        vote=None if rng.random() < 0.5 else dict(
            params=dict(tau_s=int(rng.choice([3, 10, 20])), tau_h_pct=int(rng.choice([20, 40])), iterations=int(rng.integers(1, 4)),
                        interpolate_=int(rng.integers(0, 2))),
            arms=dict(l1=vl1, l2=int(rng.integers(0, vl1 + 1)), tau1=vtau1, tau2=int(rng.integers(1, vtau1 + 1)))),
        adjust=None if rng.random() < 0.5 else dict(tau_e=int(rng.integers(1, 5)), vertical=int(rng.integers(0, 2)),
                                                    iterations=int(rng.integers(1, 9))),
        wmf=(None, "occluded", "all")[int(rng.integers(0, 3))],
        sif=int(rng.integers(1, D + 1)), bound=int(rng.choice([0, 1, 3, 7, 8, 9, D])), volumes=volumes)
    if cost != "mi":
        opt["mi"] = None
    for k in ("cross_scale", "permeability"):
        if FAMILIES[fam][2] != k:
            opt[k] = None
    return opt


def table_composition(seed, base=None):
    """the case of a seed: the walk's (family, cost, entry), and behind it an option set redrawn from the seed's stream until
    table_refusals finds nothing (PatchMatch stereo refuses most of what is drawn behind the winners)"""
    s = table_setup(base)
    w, h, D = s["w"], s["h"], s["D"]
    rng = np.random.default_rng((TABLE_BASE if base is None else int(base)) + 1 + int(seed))
    fam, cost, entry, volumes = TABLE_WALK[seed % TABLE_SEEDS]
    mi_init = sum(k[1] == "mi" for k in TABLE_WALK[:seed % TABLE_SEEDS]) % 2          # random, reference, random, ...
    while True:
        c = dict(s, opt=_table_options(rng, s, fam, cost, volumes, mi_init), entry=entry)
        if not table_refusals(c):
            break
    o = c["opt"]
    dminl, dminr = int(-rng.integers(0, D + 3)), int(rng.integers(-3, 4))
    ch = int(rng.choice([3, 4]))
    rgb = pair_steps(rng, (1, 0, 1, 2)[seed % 4], w, h, D, ch)              # (mostly textured: the depth steps have to be found)
    agg = FAMILIES[fam][0]
    shown = [k for k in ("census", "adcensus", "mi") if cost.startswith(k)] + \
            [k for k in ("sgm", "cross", "scanline", "bp", "patchmatch") if k in agg.split("-")] + \
            ["cross_scale", "permeability", "subpixel", "uniqueness", "speckle", "vote", "adjust", "wmf"]
    on = " ".join(f"{k} {o[k]}" for k in shown if o[k] is not None)
    order = [int(i) for i in rng.permutation(len(TABLE_SETTERS))]
    c.update(dminl=dminl, dminr=dminr, ch=ch, rgb=rgb, order=order,
             text=f"{w}x{h}x{D} ch {ch} radius {s['radius']} eps {s['eps']} {fam} / {cost} / {entry} entry: {on} "
                  f"dmin {dminl},{dminr} sif {o['sif']} bound {o['bound']} volumes {int(o['volumes'])}")
    return c


def table_order(base=None, count=TABLE_SEEDS):
    """the order in which the second pass over a base's context takes the seeds 0 .. count - 1"""
    rng = np.random.default_rng([TABLE_BASE if base is None else int(base), count])
    return [int(i) for i in rng.permutation(count)]


def table_applied_order(c):
    """The setters' names in the order a case applies them: the drawn permutation, except that of the three setters of the cost
    the one that switches the drawn cost on takes the last of their three places -- each of them replaces what the others
    chose, so in any other place it would be undone."""
    order = [TABLE_SETTERS[i] for i in c["order"]]
    active = {"census": "cost", "reference": "cost", "mi": "mi"}.get(c["opt"]["cost"], "adcensus")
    trio = [i for i, k in enumerate(order) if k in ("cost", "adcensus", "mi")]
    for i, k in zip(trio, [order[i] for i in trio if order[i] != active] + [active]):
        order[i] = k
    return order


def table_guides(c, front="context"):
    """Which stages take the colour pair as their guide.  The context (ctx_enqueue): cross-based aggregation, the scan-line
    optimiser and the vote wherever the pair came through the rgb entry, the permeability filter only under colour guidance.
    PairPipeline has no entry: run() takes the colour pair only where colour guidance, cross, scanline, PatchMatch or the colour
    AD term asks for one, and its vote takes the colour image exactly then."""
    o = c["opt"]
    agg, cgf, _ = FAMILIES[o["family"]]
    came = c["entry"] == "rgb"
    if front == "pipeline":
        came = came and (cgf or agg in ("cross", "scanline", "cross-scanline", "patchmatch") or o["cost"] == "adcensus colour")
    return dict(came=came, cross=came, scanline=came, vote=came, permeability=cgf)


def _table_costs(c, orc, P, kind, gray, rgb, size_d, dmin, T):
    """both views' cost volumes of `kind` on the images of one level"""
    import adcensus_ref
    import mi_ref
    o = c["opt"]
    out = []
    for v in (0, 1):
        if kind == "reference":
            out.append(orc.cost_volume(gray[v], gray[1 - v], size_d, dmin[v], params=P))
        elif kind == "census":
            out.append(census_ref.census_cost(gray[v], gray[1 - v], size_d, dmin[v], **o["census"]))
        elif kind == "mi":
            out.append(mi_ref.cost(T, gray[0], gray[1], size_d, dmin[v], right=bool(v)))
        else:
            colour = int(kind == "adcensus colour")
            img = rgb if colour else gray
            out.append(adcensus_ref.cost(img[v], img[1 - v], gray[v], gray[1 - v], size_d, dmin[v], colour=colour, **o["census"],
                                         **o["adcensus"]))
    return out


def _table_guided(c, orc, P, gray, rgb, cost, dmin):
    import cgf_ref
    if FAMILIES[c["opt"]["family"]][1]:
        return [cgf_ref.aggregate(rgb[v], cost[v], c["radius"], c["eps"]) for v in (0, 1)]
    return [orc.guided_filter(gray[v], cost[v], dmin[v], want_agg=True, params=P)[3] for v in (0, 1)]


def _table_winners(c, orc, P, gray, kind, cost=None, T=None):
    """The chain of ctx_enqueue up to the winners for the cost `kind` (or the given level-0 volumes): cost, aggregation,
    cross-scale or permeability, winners and states.  -> dict with the volumes, the planes up to dmapl / dmapr and "st"."""
    import bp_ref
    import cgf_ref
    import cscale_ref
    import patchmatch_ref
    import perm_ref
    import scanline_ref
    import sgm_ref
    import subpix_ref
    o, D, w, h = c["opt"], c["D"], c["w"], c["h"]
    agg, _, extra = FAMILIES[o["family"]]
    dmin = (c["dminl"], c["dminr"])
    rgb = c["rgb"]
    guides = table_guides(c)
    e = dict(grayl=gray[0], grayr=gray[1])
    if agg == "patchmatch":
        pm = patchmatch_ref.patchmatch(gray[0], gray[1], D, dmin[0], dmin[1], patchmatch_ref.PMParams(**o["patchmatch"]),
                                       patchmatch_ref.cost_const(P.alpha, P.th_color, P.th_grad))
        e.update(bestl=pm["cost"][0], bestr=pm["cost"][1], dmapl=pm["label"][0], dmapr=pm["label"][1], pm_planes=pm["planes"],
                 subpixl=pm["disp"][0], subpixr=pm["disp"][1], st=None)
        return e
    if cost is None:
        cost = _table_costs(c, orc, P, kind, gray, rgb, D, dmin, T)
    with np.errstate(all="ignore"):
        if agg == "guided":
            q = _table_guided(c, orc, P, gray, rgb, cost, dmin)
        elif agg == "sgm":
            q = [sgm_ref.aggregate(v, **o["sgm"]).astype(F32) for v in cost]
        elif agg == "bp":
            q = [bp_ref.outputs(v, **o["bp"])["agg"] for v in cost]
        else:
            g = rgb if guides["cross"] else gray
            vol = [cross_ref.aggregate(g[v], cost[v], **o["cross"]) for v in (0, 1)] if agg != "scanline" else cost
            q = vol if agg == "cross" else \
                [scanline_ref.outputs(g[v], g[1 - v], vol[v], dmin[v], **o["scanline"])["agg"] for v in (0, 1)]
        if extra:
            e["plainl"], e["plainr"] = q
        if extra == "cross_scale":
            scales, lam = o["cross_scale"]["scales"], o["cross_scale"]["lambda_"]
            pg = [cscale_ref.pyramid(g, scales) for g in gray]
            pc = [cscale_ref.pyramid(i, scales) for i in rgb] if guides["came"] else None
            levels = ([q[0]], [q[1]])
            e["child_size_d"] = []
            for s in range(1, scales):
                geo = [cscale_ref.level(w, h, dmin[v], D, s) for v in (0, 1)]
                sd, ds = max(geo[0][3], geo[1][3]), (geo[0][2], geo[1][2])
                e["child_size_d"].append(sd)
                gs, cs = (pg[0][s], pg[1][s]), (pc[0][s], pc[1][s]) if pc else None
                qs = _table_guided(c, orc, P, gs, cs, _table_costs(c, orc, P, kind, gs, cs, sd, ds, T), ds)
                for v in (0, 1):
                    levels[v].append(qs[v][:geo[v][3]])
            q = [cscale_ref.combine(levels[v], dmin[v], D, lam) for v in (0, 1)]
        if extra == "permeability":
            g = rgb if guides["permeability"] else gray
            q = [perm_ref.filter_volume(q[v], g[v], o["permeability"]["sigma"]) for v in (0, 1)]
    st = [cgf_ref.states(v) for v in q]
    assert all((s["z"] >= 0).all() for s in st)
    e.update(aggl=q[0], aggr=q[1], costl=cost[0], costr=cost[1], bestl=st[0]["best"], bestr=st[1]["best"],
             dmapl=subpix_ref.dmap_of(st[0]["z"], st[0]["best"], dmin[0]),
             dmapr=subpix_ref.dmap_of(st[1]["z"], st[1]["best"], dmin[1]), keys=np.stack([s["keys"] for s in st]), st=st)
    return e


def table_behind(c, orc, e, front="context"):
    """The chain of ctx_enqueue behind the winners, into `e` (of _table_winners): the LR check, uniqueness, speckle removal, the
    vote, the fill behind each outlier stage, the sub-pixel fit, the adjustment on the left volume, and the weighted median
    that PairPipeline has on top.  front: whose rule picks the guide of the vote (table_guides)."""
    import ctypes
    import adjust_ref
    import main_harness
    import subpix_ref
    import uniq_ref
    import vote_ref
    import wmf_ref
    o, D, d_lo = c["opt"], c["D"], c["dminl"]
    P = orc.Params()
    orc.lib().orc_default_params(ctypes.byref(P))
    st = e["st"]
    kw = dict(uniqueness=o["uniqueness"], speckle=o["speckle"])
    if st:
        kw.update(z=st[0]["z"], best=st[0]["best"], sec=st[0]["uq"][0], nbr=st[0]["nbr"], subpixel=o["subpixel"])
    if o["vote"]:
        guide = c["rgb"][0] if table_guides(c, front)["vote"] else e["grayl"]
        vote_ref.chain(orc, e, d_lo, D, guide, o["vote"]["params"], arms=o["vote"]["arms"], d_lr=int(P.d_lr), **kw)
    else:
        main_harness.finish_chain(orc, e, d_lo, D, **kw)
    kept = e["despeckled"] if o["speckle"] else e["unique"] if o["uniqueness"] else e["occlusion"]
    if o["uniqueness"]:
        e["margin"] = uniq_ref.apply(e["occlusion"], st[0]["z"] >= 0, st[0]["best"], st[0]["uq"][0],
                                     ratio_of(o["uniqueness"]), d_lo, d_lo - 100)[1]
    if st is None:          # PatchMatch stereo: the left disp where the pixel was kept, the filled label elsewhere
        e["subpix_filled"] = np.where(subpix_ref.kept(kept, d_lo), e["subpixl"], e["filled"]).astype(F32)
    elif o["subpixel"]:
        mode = subpix_ref.MODES[o["subpixel"]]
        for v, k in enumerate(("subpixl", "subpixr")):
            e[k], _ = subpix_ref.maps(mode, st[v]["z"], st[v]["best"], st[v]["nbr"][0], st[v]["nbr"][1], e["dmap" + "lr"[v]])
    if o["adjust"]:
        e["before"] = e["filled"]
        if o["subpixel"]:
            e["filled"], e["sub_filled"] = adjust_ref.adjust(e["before"], e["aggl"], d_lo, mode=subpix_ref.MODES[o["subpixel"]],
                                                             sub=e["sub_filled"], **o["adjust"])
        else:
            e["filled"] = adjust_ref.adjust(e["before"], e["aggl"], d_lo, **o["adjust"])
        e["adjusted"] = e["filled"]
    if st and o["subpixel"]:
        e["subpix_filled"] = e["sub_filled"]
    if o["wmf"]:
        e["refined"] = wmf_ref.weighted_median(e["grayl"], e["filled"], d_lo, D, kept if o["wmf"] == "occluded" else None)
    return e


def table_reference(c, orc, front="context"):
    """The numpy chain of a drawn table composition, in the order of ctx_enqueue; under the MI cost mi_ref.pair_loop around it,
    whose passes before the last stop behind the LR check and the fill, as ctx_pair's `early` plan does.  -> dict named like
    PairPipeline.results() plus the getters' maps (margin, mi_table, mi_hist, pm_planes); "mi_tables" are the tables of every
    pass, "plainl" / "plainr" the guided filter's volumes under cross-scale or the permeability filter."""
    import ctypes
    import mi_ref
    o, D = c["opt"], c["D"]
    P = orc.Params()
    orc.lib().orc_default_params(ctypes.byref(P))
    P.radius, P.eps = c["radius"], c["eps"]
    gray = [orc.gray(i, params=P) for i in c["rgb"]]
    if o["cost"] != "mi":
        return table_behind(c, orc, _table_winners(c, orc, P, gray, o["cost"]), front)
    mark = F32(c["dminl"] - 100)
    state = {}

    def solve(cl, cr):
        # (the levels of a cross-scale pass build their own cost: from the table of the map this pass started from)
        kind = state.pop("kind", "mi")
        T = None
        if kind == "mi" and o["cross_scale"]:
            T = mi_ref.table(mi_ref.histogram(gray[0], gray[1], state["current"], mark))
        e = _table_winners(c, orc, P, gray, kind, cost=[cl, cr], T=T)
        e["occlusion"] = orc.detect_occlusion(e["dmapl"], e["dmapr"], c["dminl"] - 100)
        state["current"] = e["occlusion"]
        return e

    def reference_costs():
        state["kind"] = "reference"
        return _table_costs(c, orc, P, "reference", gray, c["rgb"], D, (c["dminl"], c["dminr"]), None)

    if o["mi"]["init"] == mi_ref.INIT_RANDOM:
        state["current"] = mi_ref.random_map(c["w"], c["h"], c["dminl"], D, o["mi"]["seed"])
    passes = mi_ref.pair_loop(gray[0], gray[1], D, c["dminl"], c["dminr"], solve, o["mi"]["iterations"], o["mi"]["init"],
                              o["mi"]["seed"], reference_costs)
    e = passes[-1]
    e["mi_tables"] = [p["table"] for p in passes]
    e["mi_table"], e["mi_hist"] = e.pop("table"), e.pop("hist")
    return table_behind(c, orc, e, front)


def draw(stage, seed, base=None):
    return DRAW[stage](seed, base)


# ---------------------------------------------------------------------------------------------
# the checks of include/smx.h, mirrored: a draw that one of these refuses would be refused by its entry
# ---------------------------------------------------------------------------------------------
def _finite(x):
    return bool(np.isfinite(x))


def census_ok(rx, ry, th):
    return 1 <= rx <= 4 and 1 <= ry <= 3 and th >= 1


def accepted(stage, c):
    """the argument checks of the stage's device entries on the drawn case"""
    ok = c["w"] >= 1 and c["h"] >= 1 and c["w"] * c["h"] < 2 ** 31
    if stage == "census":
        return ok and census_ok(c["rx"], c["ry"], c["th"]) and 0 <= c["s0"] <= c["s1"] <= c["D"]
    if stage == "adcensus":
        return ok and census_ok(c["rx"], c["ry"], c["th"]) and 0 <= c["s0"] <= c["s1"] <= c["D"] and \
            all(_finite(c[k]) and 0 < c[k] <= 1e6 for k in ("lambda_census", "lambda_ad")) and \
            _finite(c["scale"]) and 2.0 ** -20 <= c["scale"] <= 2.0 ** 20 and c["colour"] in (0, 1) and \
            c["ch"] in ((3, 4) if c["colour"] else (1,))
    if stage in ("cgf", "cross"):
        f = c["form"]
        ok = ok and c["D"] >= 1 and 1 <= f["c"] <= c["D"] and f["bound"] >= 0 and f["ranges"][0][0] == 0 and \
            f["ranges"][-1][1] == c["D"] and all(a < b for a, b in f["ranges"]) and \
            all(f["ranges"][i][1] == f["ranges"][i + 1][0] for i in range(len(f["ranges"]) - 1))
        if stage == "cgf":
            return ok and c["ch"] in (3, 4) and c["radius"] >= 0 and c["h"] <= 65535 and _finite(c["eps"])
        return ok and c["ch"] in (1, 3, 4) and cross_ref.params_ok(c["l1"], c["l2"], c["tau1"], c["tau2"], c["iterations"])
    if stage == "sgm":
        return ok and 1 <= c["D"] <= 256 and 0 <= c["p1"] <= c["p2"] <= 4095 and c["paths"] in (4, 8)
    if stage == "wta":
        p = c["params"]
        return ok and c["w"] >= 2 and c["D"] >= 1 and p["radius"] >= 0 and (c["path"] != 5 or (p["radius"] == 9 and 1 <= p["eps"] < 1e30 and 0 <= p["alpha"] <= 1 and p["th_grad"] <= 2048)) and \
            (c["path"] != 3 or p["radius"] <= 9) and p["th_color"] <= 59744 and p["th_grad"] <= 59872 and \
            _finite(c["ratio"]) and c["ratio"] >= 0
    if stage == "speckle":
        return ok and c["max_size"] >= 0 and _finite(c["max_diff"]) and c["max_diff"] >= 0
    if stage == "wmf":
        return ok and 1 <= c["radius"] <= 15 and all(_finite(c[k]) and c[k] > 0 for k in ("sigma_s", "sigma_c")) and \
            1 <= c["D"] <= 4096
    if stage == "mi":
        return ok and c["D"] >= 1 and 0 <= c["s0"] <= c["s1"] <= c["D"] and c["views"] in ("both", "left", "right")
    if stage == "patchmatch":
        pm = c["pm"]
        return ok and c["w"] < 2 ** 24 and 1 <= c["D"] <= 2 ** 20 and abs(c["dminl"]) <= 2 ** 20 and \
            abs(c["dminr"]) <= 2 ** 20 and 0 <= pm["radius"] <= 17 and _finite(pm["gamma"]) and pm["gamma"] > 0 and \
            1 <= pm["iterations"] <= 16 and \
            0 <= pm["max_slope"] <= 8
    if stage == "bp":
        return ok and 1 <= c["D"] <= 256 and 0 <= c["step"] <= 4095 and 0 <= c["trunc"] <= 4095 and 0 <= c["iterations"] <= 64 and \
            1 <= c["levels"] <= 8 and _finite(c["data_scale"]) and c["data_scale"] > 0
    if stage == "permeability":
        return ok and 1 <= c["D"] <= 2 ** 20 and c["ch"] in (1, 3, 4) and _finite(c["sigma"]) and c["sigma"] > 0 and \
            c["views"] in ("both", "left", "right") and c["store"] in PERM_STORES and \
            (c["c"] is None or 1 <= c["c"] <= c["D"]) and \
            c["bound"] >= 0
    raise KeyError(stage)


# ---------------------------------------------------------------------------------------------
# what a drawn case has to give: the stages' numpy references (and the oracle for the reference's own aggregation)
# ---------------------------------------------------------------------------------------------
def _views(views):
    return {"both": (0, 1), "left": (0,), "right": (1,)}[views]


def reference(stage, c, orc=None, tables=None):
    """dict of the expected outputs of the drawn case; per-view entries are lists over both views, whatever the call takes.
    orc: the oracle module, for "wta".  tables: (spatial, range) of "wmf" instead of wmf_ref.weight_tables."""
    import adcensus_ref
    import cgf_ref
    import sgm_ref
    import speckle_ref
    import uniq_ref
    import wmf_ref
    if stage == "census":
        codes = [census_ref.census_transform(i, c["rx"], c["ry"]) for i in (c["Il"], c["Ir"])]
        cost = [census_ref.cost_from_codes(codes[v], codes[1 - v], c["D"], (c["dminl"], c["dminr"])[v], c["rx"], c["ry"], c["th"],
                                           c["s0"], c["s1"]) for v in (0, 1)]
        return dict(codes=codes, cost=cost)
    if stage == "adcensus":
        kw = {k: c[k] for k in ("rx", "ry", "th", "lambda_census", "lambda_ad", "scale", "colour")}
        return dict(cost=[adcensus_ref.cost(c["imgs"][v], c["imgs"][1 - v], c["grays"][v], c["grays"][1 - v], c["D"],
                                            (c["dminl"], c["dminr"])[v], s_begin=c["s0"], s_end=c["s1"], **kw) for v in (0, 1)])
    if stage in ("cgf", "cross"):
        with np.errstate(all="ignore"):
            if stage == "cgf":
                q = [cgf_ref.aggregate(c["guides"][v], c["costs"][v], c["radius"], c["eps"]) for v in (0, 1)]
                out = {}
            else:
                kw = {k: c[k] for k in ("l1", "l2", "tau1", "tau2")}
                arms = [cross_ref.arms(g, **kw) for g in c["guides"]]
                q = []
                for v in (0, 1):                      # cross_ref.aggregate_int on the arms above, not computed twice
                    ar, V = cross_ref.areas(arms[v]), 16 * cross_ref.clamp_cost(c["costs"][v])
                    for i in range(c["iterations"]):
                        V = cross_ref.iterate(V, arms[v], ar, i)
                    q.append((V.astype(F32) * F32(0.0625)).astype(F32))
                out = dict(arms=arms)
            out.update(q=q, states=[cgf_ref.states(v) for v in q])
        return out
    if stage == "sgm":
        outs = [sgm_ref.outputs(v, c["p1"], c["p2"], c["paths"]) for v in c["costs"]]
        for o in outs:
            _, _, sec, rest, last, _ = uniq_ref.second_best(o["agg"])
            o["uq"] = np.stack((sec, rest, last)).astype(F32)
        return dict(views=outs)
    if stage == "wta":
        import ctypes
        P = orc.Params()
        orc.lib().orc_default_params(ctypes.byref(P))
        for k, v in c["params"].items():
            setattr(P, k, v)
        with np.errstate(all="ignore"):
            r = orc.stereo_pair(c["Il"], c["Ir"], c["D"], dminl=c["dminl"], dminr=c["dminr"], want_agg=True, params=P)
            r["states"] = [cgf_ref.states(r[k]) for k in ("aggl", "aggr")]
        return r
    if stage == "speckle":
        return dict(out=speckle_ref.speckle_filter(c["disp"], c["dmin"], c["dmin"] - 100, c["max_size"], c["max_diff"]))
    if stage == "mi":
        import mi_ref
        H = mi_ref.histogram(c["Il"], c["Ir"], c["disp"], c["mark"])
        learned = mi_ref.table(H)
        T = learned if c["table"] == "learned" else c["asym"]
        return dict(hist=H, learned=learned, table=T,
                    random_map=mi_ref.random_map(c["w"], c["h"], c["dminl"], c["D"], c["map_seed"]),
                    cost=[mi_ref.cost(T, c["Il"], c["Ir"], c["D"], (c["dminl"], c["dminr"])[v], bool(v), c["s0"], c["s1"])
                          for v in (0, 1)])
    if stage == "patchmatch":
        import ctypes
        import patchmatch_ref
        if orc is None:
            import oracle as orc
        P = orc.Params()
        orc.lib().orc_default_params(ctypes.byref(P))
        pm, cc = patchmatch_ref.PMParams(**c["pm"]), patchmatch_ref.cost_const(P.alpha, P.th_color, P.th_grad)
        if c["entry"] == "search":
            return patchmatch_ref.patchmatch(c["left"], c["right"], c["D"], c["dminl"], c["dminr"], pm, cc)
        views = ((c["left"], c["right"], c["dminl"]), (c["right"], c["left"], c["dminr"]))
        return dict(cost=np.stack([patchmatch_ref.plane_cost_map(own, other, dmin, c["D"], pm, cc, c["planes"][v])
                                   for v, (own, other, dmin) in enumerate(views)]))
    if stage == "bp":
        import bp_ref
        return dict(views=[bp_ref.outputs(v, c["step"], c["trunc"], c["iterations"], c["levels"], c["data_scale"])
                           for v in c["costs"]])
    if stage == "permeability":
        import perm_ref
        import subpix_ref
        views = []
        for v in (0, 1):
            out = perm_ref.filter_volume(c["costs"][v], c["guides"][v], c["sigma"])
            z, c0, lo, hi, last = subpix_ref.winners(out)
            _, _, sec, rest, last_u, _ = uniq_ref.second_best(out)
            views.append(dict(out=out, keys=perm_ref.pack_keys(z, c0), nbr=np.stack([lo, hi, last]).astype(F32),
                              uq=np.stack([sec, rest, last_u]).astype(F32)))
        return dict(views=views)
    if stage == "wmf":
        ws, wc = tables if tables is not None else wmf_ref.weight_tables(c["radius"], c["sigma_s"], c["sigma_c"])
        return dict(out=wmf_ref.weighted_median(c["guide"], c["disp"], c["dmin"], c["D"], c["select"], c["radius"], ws, wc))
    raise KeyError(stage)
