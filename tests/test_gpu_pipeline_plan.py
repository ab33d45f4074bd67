"""A PairPipeline owns what its plan says, and nothing else: for a dozen configurations that between them switch every row of
pipeline_plan.STAGES on, every buffer of the plan is on the object with the planned shape, dtype and device, every other buffer
attribute is None, self.mean is zero where the plan says so, and run() then results() returns the keys the plan implies.  At
w=33, h=9, size_d=5 with two slices in flight the chunk buffers exist and the last chunk is short.  No numerics here: that is
the rest of the suite's job."""
import numpy as np
import pytest
import torch

import stereo_matching_cuda_amd as smx
from stereo_matching_cuda_amd import pipeline_plan as pp
from stereo_matching_cuda_amd.device import PairPipeline

pytestmark = pytest.mark.gpu

W, H, D, SIF = 33, 9, 5, 2
BASE_KEYS = {"bestl", "bestr", "dmapl", "dmapr", "meanl", "meanr", "occlusion", "filled"}
# what results() returns for a row that is on, beside BASE_KEYS
ROW_KEYS = {"want_agg": {"aggl", "aggr"}, "adjust": {"aggl", "aggr", "adjusted"}, "cross_scale": {"aggl", "aggr"},
            "permeability": {"aggl", "aggr"}, "wmf": {"refined"}, "uniqueness": {"unique", "margin"}, "speckle": {"despeckled"},
            "vote": {"voted"}, "subpixel": {"subpixl", "subpixr", "subpix_filled"},
            "patchmatch": {"pm_planes", "subpixl", "subpixr", "subpix_filled"}}


def _colour():
    p = smx.default_adcensus_params()
    p.colour = 1
    return p


def _two_scales():
    p = smx.default_cscale_params()
    p.scales = 2
    return p


def _one_iteration():
    p = smx.default_mi_params()
    p.iterations = 1
    return p


CONFIGS = {
    "plain": dict(),
    "census, every outlier stage": dict(cost="census", want_agg=True, uniqueness=0.25, subpixel="parabola", speckle=True, vote=True,
                                        wmf="occluded"),
    "adcensus with colour": dict(cost="adcensus", adcensus_params=_colour(), want_agg=True, subpixel="equiangular"),
    "mi": dict(cost="mi", mi_params=_one_iteration(), wmf="all"),
    "rgb, adjust": dict(guidance="rgb", adjust=True),
    "cross-scale, two scales": dict(cross_scale=_two_scales(), guidance="rgb", cost="adcensus", uniqueness=0.5),
    "permeability": dict(permeability=True, cost="census", subpixel="parabola"),
    "sgm": dict(aggregation="sgm", cost="census", uniqueness=0.25, want_agg=True),
    "bp": dict(aggregation="bp", speckle=True),
    "cross": dict(aggregation="cross", want_agg=True, vote=True),
    "scanline": dict(aggregation="scanline", adjust=True, subpixel="parabola"),
    "cross-scanline with want_agg": dict(aggregation="cross-scanline", want_agg=True, cost="census"),
    "patchmatch": dict(aggregation="patchmatch", speckle=True, vote=True, wmf="all"),
}


def test_the_configurations_switch_every_row_on():
    lib = smx.lib()
    on = set()
    for kw in CONFIGS.values():
        on |= set(pp.plan_pipeline(lib, W, H, D, slices_in_flight=SIF, **kw).on)
    assert on == {r.key for r in pp.STAGES}


def _owns_its_plan(pipe, device):
    plan = pipe.plan
    planned = {name: (shape, dtype, zeroed) for name, shape, dtype, zeroed in plan.buffers}
    for name in pp.BUFFERS:
        t = getattr(pipe, name)
        if name not in planned:
            assert t is None, name
            continue
        shape, dtype, zeroed = planned[name]
        assert tuple(t.shape) == tuple(shape) and t.dtype == getattr(torch, dtype) and t.device == device and t.is_contiguous(), name
        assert not zeroed or not bool(t.any()), name
    assert set(planned) <= set(pp.BUFFERS) and planned["mean"][2] == plan.no_walker
    for name, value in {**plan.options, **plan.bytes}.items():
        assert getattr(pipe, name) is value, name
    assert len(pipe.cs_levels) == len(pipe.cs_gray) == len(pipe.cs_rgb) == len(plan.levels)
    for k, gray, rgb, (_, sub, gray_shape, rgb_shape) in zip(pipe.cs_levels, pipe.cs_gray, pipe.cs_rgb, plan.levels):
        assert tuple(gray.shape) == gray_shape and gray.dtype == torch.uint8 and gray.device == device
        assert (rgb is None) == (rgb_shape is None)
        assert rgb is None or (tuple(rgb.shape) == rgb_shape and rgb.dtype == torch.uint8 and rgb.device == device)
        assert k.plan is sub
        _owns_its_plan(k, device)
        for name in pp.LEVEL_SHARES:            # (the level's plan has one of its own shape: it is level 0's)
            assert getattr(k, name) is getattr(pipe, name)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_a_pipeline_owns_what_its_plan_says_and_returns_the_keys_it_implies(name):
    kw = CONFIGS[name]
    device = torch.device("cuda:0")
    pipe = PairPipeline(W, H, D, slices_in_flight=SIF, device=device, **kw)
    plan = pp.plan_pipeline(smx.lib(), W, H, D, slices_in_flight=SIF, **kw)
    assert pipe.slices_in_flight == plan.slices_in_flight == SIF
    assert (pipe.plan.on, pipe.plan.bytes, pipe.plan.buffers, pipe.plan.no_walker) == (plan.on, plan.bytes, plan.buffers, plan.no_walker)
    assert [lv[2:] for lv in pipe.plan.levels] == [lv[2:] for lv in plan.levels]
    _owns_its_plan(pipe, device)
    # the chunk buffers are there where the configuration runs chunks and keeps volumes, and the last chunk is short
    assert D % SIF == 1
    planned = {b[0] for b in plan.buffers}
    assert ("_agg_chunk" in planned) == (name in ("census, every outlier stage", "adcensus with colour", "rgb, adjust", "cross-scale, two scales",
                                                  "permeability", "cross"))
    assert ("_so_chunk" in planned) == (name == "cross-scanline with want_agg")
    rng = np.random.default_rng(7)
    rgb = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    gray = torch.from_numpy(np.ascontiguousarray(rgb[..., 1])).to(device)
    colour = torch.from_numpy(rgb).to(device)
    needs_colour = "rgb" in plan.on or (pipe.cost == "adcensus" and bool(pipe.adcensus_params.colour))
    if needs_colour:
        pipe.run(gray[0], gray[1], rgb_l=colour[0], rgb_r=colour[1])
    else:
        pipe.run(gray[0], gray[1])
    want = set(BASE_KEYS)
    for key in plan.on:
        want |= ROW_KEYS.get(key, set())
    got = pipe.results()
    assert set(got) == want
    assert all(isinstance(v, np.ndarray) for v in got.values())
    # nothing was allocated or dropped by the run, and a pipeline without mean images still has them zero
    _owns_its_plan(pipe, device)
