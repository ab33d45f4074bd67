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
"""
import numpy as np

import census_ref
import cross_ref

F32 = np.float32
STAGES = ("census", "adcensus", "cgf", "cross", "sgm", "wta", "speckle", "wmf")
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


DRAW = dict(census=census, adcensus=adcensus, cgf=cgf, cross=cross, sgm=sgm, wta=wta, speckle=speckle, wmf=wmf)


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
    if stage == "wmf":
        ws, wc = tables if tables is not None else wmf_ref.weight_tables(c["radius"], c["sigma_s"], c["sigma_c"])
        return dict(out=wmf_ref.weighted_median(c["guide"], c["disp"], c["dmin"], c["D"], c["select"], c["radius"], ws, wc))
    raise KeyError(stage)
