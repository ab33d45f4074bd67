"""Cross-scale cost aggregation on the CPU: the properties of the numpy reference tests/cscale_ref.py (weights, level geometry,
pyramid), and what the method buys on a scene with a textureless band wider than the guided filter's window, with every level's
aggregated volumes from the CPU oracle.

The scene (192 x 48, size_d 16, dminl -15, dminr 0, default parameters): base = default_rng(seed).integers(0, 256, (48, 224)),
columns [76, 76 + B) of it set to 128 -- a textureless band at columns [60, 60 + B) of the left image -- L = base[:, 16:208],
R = base[:, 16 + d:208 + d], independent normal(0, 1) noise on L, then on R, clipped, rounded, u8.  The true left label is -d.

Figures of the committed reference, seeds 0 / 1, d 6, B 60, 4 scales, lambda 1.0, pixels of the band (2880) off by more than 1:
    fine scale alone  1061 / 753        cross-scale  0 / 0
and columns 20..59 (textured) have no wrong pixel in either map.  Exact-label errors inside the band stay high with
cross-scale on (875 / 734): a label of level s stands for 2^s labels of level 0.
"""
import numpy as np
import pytest

import cscale_ref as ref

F32 = np.float32


# ---------------------------------------------------------------------------------------------
# weights
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", [0.3, 1.0, 2.5])
def test_weights_against_hand_inverted_matrices(lam):
    # 2 x 2: [[1+l, -l], [-l, 1+l]], det = 1 + 2l
    det = 1 + 2 * lam
    np.testing.assert_allclose(ref.weights(2, lam), [(1 + lam) / det, lam / det], rtol=1e-6)
    # 3 x 3: [[1+l, -l, 0], [-l, 1+2l, -l], [0, -l, 1+l]]: row 0 of the adjugate over the determinant
    a, b = 1 + lam, 1 + 2 * lam
    det = a * (b * a - lam * lam) - lam * lam * a
    np.testing.assert_allclose(ref.weights(3, lam), [(b * a - lam * lam) / det, lam * a / det, lam * lam / det], rtol=1e-6)


@pytest.mark.parametrize("scales", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("lam", [0.0, 0.3, 1.0, 7.0])
def test_weights_are_row_0_of_the_inverse_and_sum_to_1(scales, lam):
    wt = ref.weights(scales, lam)
    assert wt.dtype == F32 and wt.shape == (scales,)
    np.testing.assert_allclose(wt, np.linalg.inv(ref.matrix(scales, lam))[0], rtol=1e-6, atol=1e-12)
    assert abs(float(wt.astype(np.float64).sum()) - 1.0) <= 1e-6
    if scales == 1:
        assert wt.tolist() == [1.0]
    if lam == 0.0:
        assert wt.tolist() == [1.0] + [0.0] * (scales - 1)


# ---------------------------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dmin", [-15, -16, -1, 0, 3])
@pytest.mark.parametrize("size_d", [1, 2, 16, 17])
def test_every_label_has_its_ancestor_and_both_ends_are_reached(dmin, size_d):
    for s in range(ref.MAX_SCALES):
        _, _, lo, ds = ref.level(19, 40, dmin, size_d, s)
        anc = [((dmin + z) >> s) - lo for z in range(size_d)]
        assert min(anc) == 0 and max(anc) == ds - 1
        assert all(0 <= a < ds for a in anc)
        assert lo == int(np.floor(dmin / 2.0 ** s))


def test_level_sizes_halve_rounding_up():
    assert ref.level(19, 40, 0, 1, 4)[:2] == (2, 3)
    assert ref.level(129, 70, 0, 1, 3)[:2] == (17, 9)
    assert ref.level(1, 1, 0, 1, 4)[:2] == (1, 1)


# ---------------------------------------------------------------------------------------------
# pyramid
# ---------------------------------------------------------------------------------------------
def _pyr_down_loops(img):
    """the definition as a direct five-tap double loop"""
    h, w = img.shape
    tap = [1, 4, 6, 4, 1]

    def at(i, n):
        i = -i if i < 0 else i
        i = 2 * (n - 1) - i if i >= n else i
        return min(max(i, 0), n - 1)
    out = np.zeros(((h + 1) // 2, (w + 1) // 2), np.uint8)
    for yo in range(out.shape[0]):
        for xo in range(out.shape[1]):
            t = 0
            for j in range(5):
                for i in range(5):
                    t += tap[j] * tap[i] * int(img[at(2 * yo - 2 + j, h), at(2 * xo - 2 + i, w)])
            out[yo, xo] = (t + 128) >> 8
    return out


@pytest.mark.parametrize("w,h", [(1, 1), (2, 1), (1, 2), (5, 3)])
def test_pyr_down_matches_the_double_loop(w, h):
    img = np.random.default_rng(w * 10 + h).integers(0, 256, (h, w)).astype(np.uint8)
    assert np.array_equal(ref.pyr_down(img), _pyr_down_loops(img))
    rgb = np.random.default_rng(w * 10 + h + 1).integers(0, 256, (h, w, 3)).astype(np.uint8)
    got = ref.pyr_down(rgb)
    for c in range(3):
        assert np.array_equal(got[:, :, c], _pyr_down_loops(rgb[:, :, c]))


@pytest.mark.parametrize("value", [0, 1, 128, 255])
def test_pyr_down_of_a_constant_image_is_constant(value):
    for shape in ((1, 1), (2, 5), (7, 6), (7, 6, 4)):
        out = ref.pyr_down(np.full(shape, value, np.uint8))
        assert out.shape[:2] == ((shape[0] + 1) // 2, (shape[1] + 1) // 2) and (out == value).all()


# ---------------------------------------------------------------------------------------------
# combination
# ---------------------------------------------------------------------------------------------
def _random_levels(rng, w, h, dmin, size_d, scales):
    return [rng.standard_normal((ref.level(w, h, dmin, size_d, s)[3],) + ref.level(w, h, dmin, size_d, s)[1::-1]).astype(F32)
            for s in range(scales)]


def test_one_scale_and_lambda_0_return_level_0():
    rng = np.random.default_rng(5)
    lv = _random_levels(rng, 19, 7, -15, 16, 3)
    lv[0][3, 2, 5] = np.nan
    lv[0][4, 1, 1] = -0.0
    assert np.array_equal(ref.combine(lv[:1], -15, 16, 1.0).view(np.uint32), lv[0].view(np.uint32))
    out = ref.combine(lv, -15, 16, 0.0)
    ok = ~np.isnan(lv[0])
    assert np.array_equal(out[ok], (lv[0] + F32(0))[ok]) and np.isnan(out[~ok]).all()


def test_combination_against_a_pixel_loop():
    rng = np.random.default_rng(6)
    w, h, dmin, size_d, scales, lam = 7, 5, -3, 6, 3, 0.3
    lv = _random_levels(rng, w, h, dmin, size_d, scales)
    wt = ref.weights(scales, lam)
    out = ref.combine(lv, dmin, size_d, lam)
    for z in range(size_d):
        for y in range(h):
            for x in range(w):
                o = F32(wt[0] * lv[0][z, y, x])
                for s in range(1, scales):
                    o = F32(o + F32(wt[s] * lv[s][((dmin + z) >> s) - (dmin >> s), y >> s, x >> s]))
                assert o == out[z, y, x]


# ---------------------------------------------------------------------------------------------
# what the method buys: the textureless band
# ---------------------------------------------------------------------------------------------
W, H, D, DMINL, DMINR = 192, 48, 16, -15, 0


def scene(seed, d, B):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (H, 224)).astype(np.float64)
    base[:, 76:76 + B] = 128
    L = base[:, 16:208] + rng.normal(0, 1, (H, W))
    R = base[:, 16 + d:208 + d] + rng.normal(0, 1, (H, W))
    return tuple(np.clip(np.rint(v), 0, 255).astype(np.uint8) for v in (L, R))


def left_levels(L, R, scales):
    import oracle
    out = []
    for s, (l, r) in enumerate(zip(ref.pyramid(L, scales), ref.pyramid(R, scales))):
        _, _, dl, sl = ref.level(W, H, DMINL, D, s)
        _, _, dr, sr = ref.level(W, H, DMINR, D, s)
        out.append(oracle.stereo_pair(l, r, max(sl, sr), dminl=dl, dminr=dr, want_agg=True)["aggl"][:sl])
    return out


@pytest.fixture(scope="module", params=[0, 1])
def band(request):
    d, B, scales, lam = 6, 60, 4, 1.0
    L, R = scene(request.param, d, B)
    lv = left_levels(L, R, scales)
    fine = ref.label_map(ref.winners(lv[0])[0], DMINL)
    cross = ref.label_map(ref.winners(ref.combine(lv, DMINL, D, lam))[0], DMINL)
    return d, B, fine, cross


def _off(m, d, c0, c1, by):
    return int((np.abs(m[:, c0:c1] + d) > by).sum())


def test_cross_scale_repairs_the_band(band):
    d, B, fine, cross = band
    print("band off by more than 1: fine", _off(fine, d, 60, 60 + B, 1), "cross-scale", _off(cross, d, 60, 60 + B, 1),
          "| exact-label errors with cross-scale", _off(cross, d, 60, 60 + B, 0))
    assert _off(cross, d, 60, 60 + B, 1) == 0
    assert _off(fine, d, 60, 60 + B, 1) >= 500


def test_textured_columns_are_right_in_both_maps(band):
    d, B, fine, cross = band
    assert _off(fine, d, 20, 60, 0) == 0
    assert _off(cross, d, 20, 60, 0) == 0
