"""The mutual-information cost without a GPU: smx_mi_table (host only, through _lib) against tests/mi_ref.py, and what the
cost is for -- the scene of DESIGN.md 4.3s, a pair whose right image went through a mapping that is not increasing, run through
the numpy loop of smx_ctx_set_mi (mi_ref.pair_loop) with the oracle's guided filter as the aggregation.

Wrong labels are counted among the 7392 kept pixels on the winner-take-all left map (`dmapl`, "wta" below: the map the
feasibility check counted) and on the final filled map ("filled").  The counts are deterministic and asserted as measured.
"""
import numpy as np
import pytest

import stereo_matching_cuda_amd as smx

import adcensus_ref
import census_ref
import mi_ref as ref

D, DMINL, DMINR = ref.SCENE_D, ref.SCENE_DMIN, 0
KEPT = 7392
MAPPINGS = ("invert", "permute", "fold")


# ---------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------
def _histograms():
    Il, Ir, truth, _ = ref.scene(0, "permute")
    hs = {"scene": ref.histogram(Il, Ir, truth, DMINL - 100), "empty": np.zeros((256, 256), np.uint32)}
    hs["single cell"] = hs["empty"].copy()
    hs["single cell"][17, 200] = 12345
    hs["diagonal"] = np.diag(np.arange(1, 257, dtype=np.uint32))
    hs["uniform"] = np.full((256, 256), 3, np.uint32)
    hs["large counts"] = np.random.default_rng(4).integers(0, 1 << 32, (256, 256), dtype=np.uint64).astype(np.uint32)
    return hs


@pytest.mark.parametrize("name", ["scene", "empty", "single cell", "diagonal", "uniform", "large counts"])
def test_table_equals_the_reference(name):
    H = _histograms()[name]
    got, want = smx.mi_table(H), ref.table(H)
    assert got.dtype == np.uint8 and got.shape == (256, 256)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{name}: {bad.size} entries differ, first at {bad[:5]}"
    if name == "empty":
        assert not got.any()
    else:
        assert got.min() == 0 and got.max() == 255


def test_table_of_the_scene_is_low_where_the_pixels_correspond():
    """The cost of the pairs the true map produces is far below the cost of the pairs it never produces."""
    Il, Ir, truth, _ = ref.scene(0, "permute")
    T = smx.mi_table(ref.histogram(Il, Ir, truth, DMINL - 100)).astype(np.int64)
    m = ref.mapping("permute").astype(np.int64)
    on = T[np.arange(256), m]
    assert on.max() < 64 and np.median(T) > 128
    assert not np.array_equal(T, T.T)


def test_histogram_reference_counts_what_the_definition_says():
    Il = np.array([[1, 2, 3, 4]], np.uint8)
    Ir = np.array([[9, 8, 7, 6]], np.uint8)
    disp = np.array([[-1, -1, -50, 1]], np.float32)          # off the left edge, a partner, the mark, off the right edge
    H = ref.histogram(Il, Ir, disp, -50)
    assert H.sum() == 1 and H[2, 9] == 1


def test_params_and_defaults():
    p = smx.default_mi_params()
    assert (p.iterations, p.init, p.seed) == (3, 0, 0)


# ---------------------------------------------------------------------------------------------
# the scene
# ---------------------------------------------------------------------------------------------
def _solver(orc, Il, Ir):
    def solve(cl, cr):
        _, ml, _, _ = orc.guided_filter(Il, cl, DMINL)
        _, mr, _, _ = orc.guided_filter(Ir, cr, DMINR)
        occ = orc.detect_occlusion(ml, mr, DMINL - 100)
        return dict(dmapl=ml, dmapr=mr, occlusion=occ, filled=orc.fill_occlusion(occ, float(DMINL)))
    return solve


_COUNTS = {}


def counts(orc, mapname, seed):
    """(wta, filled) wrong-label counts per cost: 'reference', 'census', 'adcensus', and per MI init the three tables."""
    key = (mapname, seed)
    if key not in _COUNTS:
        Il, Ir, truth, kept = ref.scene(seed, mapname)
        assert int(kept.sum()) == KEPT
        solve = _solver(orc, Il, Ir)

        def both(r):
            return ref.wrong(r["dmapl"], truth, kept), ref.wrong(r["filled"], truth, kept)

        def refc():
            return orc.cost_volume(Il, Ir, D, DMINL), orc.cost_volume(Ir, Il, D, DMINR)

        row = {"reference": both(solve(*refc())),
               "census": both(solve(census_ref.census_cost(Il, Ir, D, DMINL), census_ref.census_cost(Ir, Il, D, DMINR))),
               "adcensus": both(solve(adcensus_ref.gray_cost(Il, Ir, D, DMINL), adcensus_ref.gray_cost(Ir, Il, D, DMINR)))}
        for name, init in (("mi random", ref.INIT_RANDOM), ("mi reference", ref.INIT_REFERENCE)):
            row[name] = [both(p) for p in ref.pair_loop(Il, Ir, D, DMINL, DMINR, solve, 3, init, 0, refc)]
        _COUNTS[key] = row
    return _COUNTS[key]


# (wta, filled) as measured with the oracle's guided filter (radius 9, the defaults); DESIGN.md 4.3s holds the same table
MEASURED = {
    ('invert', 0): {'reference': (7391, 7392), 'census': (7392, 7392), 'adcensus': (7392, 7392), 'mi random': [(8, 148), (0, 143), (0, 144)], 'mi reference': [(7392, 7392), (3968, 3487), (112, 140)]},
    ('invert', 1): {'reference': (7391, 7392), 'census': (7392, 7392), 'adcensus': (7392, 7392), 'mi random': [(0, 135), (0, 149), (0, 149)], 'mi reference': [(7374, 7322), (2445, 1137), (0, 148)]},
    ('permute', 0): {'reference': (7217, 7231), 'census': (6675, 6887), 'adcensus': (7312, 7392), 'mi random': [(38, 124), (0, 139), (0, 139)], 'mi reference': [(2992, 1705), (15, 161), (0, 142)]},
    ('permute', 1): {'reference': (7006, 6901), 'census': (6226, 6029), 'adcensus': (7315, 7261), 'mi random': [(4, 130), (0, 136), (0, 136)], 'mi reference': [(461, 329), (0, 139), (0, 137)]},
    ('fold', 0): {'reference': (5046, 4252), 'census': (3887, 6227), 'adcensus': (3626, 2487), 'mi random': [(8, 130), (0, 140), (0, 140)], 'mi reference': [(89, 152), (0, 140), (0, 140)]},
    ('fold', 1): {'reference': (6050, 5416), 'census': (3898, 5877), 'adcensus': (3653, 2460), 'mi random': [(0, 136), (0, 144), (0, 145)], 'mi reference': [(1297, 165), (0, 146), (0, 144)]},
}


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("mapname", MAPPINGS)
def test_scene_counts_are_the_measured_ones(orc, mapname, seed):
    row = counts(orc, mapname, seed)
    print(f"\n{mapname} seed {seed}: {row}")
    assert row == MEASURED[(mapname, seed)]


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("mapname", ["invert", "permute"])
def test_mi_finds_the_labels_where_the_other_costs_do_not(orc, mapname, seed):
    """The condition of the feature: under inversion and under the permutation, for both seeds, MI after three tables (the
    default: random start) is wrong on at most 1 % of the kept pixels, the reference cost and census each on more than half.

    The start from the reference's cost (init = reference) meets it on three of the four cases and misses it under inversion
    with seed 0: 112 of 7392 (1.5 %) after three tables, from 7392 and 3968 after one and two (MEASURED above).  Under
    inversion the reference's cost is not merely uninformed but anti-correlated -- it prefers the partner whose value differs
    most -- so its map is wrong on every kept pixel in a consistent way, the first table learns that wrong relation, and the
    loop needs a table more to leave it than it needs from a random map.  The filled map's 124 .. 149 are not labels the cost
    got wrong: they are left pixels that the LR check invalidates against the right map and the fill then takes from a
    neighbour; the plain pair (identity mapping, the reference's cost) leaves 142 and 149 of them on the same textures, with
    no wrong label on the winner-take-all map."""
    row = counts(orc, mapname, seed)
    assert row["mi random"][2][0] <= KEPT // 100
    assert row["reference"][0] > KEPT // 2 and row["census"][0] > KEPT // 2


# wta counts after tables 1, 2, 3 on the texture smoothed twice by a 5-point mean: (random start, reference start)
MEASURED_SMOOTH = {
    ('invert', 0): ([63, 3, 3], [6849, 2480, 80]),
    ('invert', 1): ([84, 2, 0], [7294, 4132, 1396]),
    ('permute', 0): ([364, 5, 5], [4, 3, 3]),
    ('permute', 1): ([459, 0, 0], [12, 0, 0]),
    ('fold', 0): ([208, 4, 5], [312, 5, 5]),
    ('fold', 1): ([193, 9, 5], [27, 3, 3]),
}


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("mapname", MAPPINGS)
def test_smoothed_texture_counts_are_the_measured_ones(orc, mapname, seed):
    """The second scene of the feasibility check: less texture, so a few pixels stay wrong and the count is not monotone from
    one table to the next (fold, seed 0: 4 then 5).  From the random start every case stays under 1 % after two tables; the
    reference start under inversion does not (80 and 1396 after three)."""
    Il, Ir, truth, kept = ref.scene(seed, mapname, smooth=2)
    solve = _solver(orc, Il, Ir)

    def refc():
        return orc.cost_volume(Il, Ir, D, DMINL), orc.cost_volume(Ir, Il, D, DMINR)

    got = tuple([ref.wrong(p["dmapl"], truth, kept) for p in ref.pair_loop(Il, Ir, D, DMINL, DMINR, solve, 3, init, 0, refc)]
                for init in (ref.INIT_RANDOM, ref.INIT_REFERENCE))
    print(f"\nsmoothed {mapname} seed {seed}: {got}")
    assert got == MEASURED_SMOOTH[(mapname, seed)]
    assert max(got[0][1:]) <= KEPT // 100
