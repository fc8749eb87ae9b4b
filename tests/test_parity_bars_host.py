"""The bars of tests/test_gpu_parity.py compare_backward, exercised on the CPU with the oracle alone.

Linearity: the masked leg's oracle side is g - g_flip in float64 (g the oracle's backward of the whole upstream
gradient, g_flip that of the upstream gradient restricted to the flip candidates), not a third backward.  It must agree
with the oracle's direct backward of the masked upstream gradient within 1e-6 relative L2 per gradient:
GRAD_CLEAN_TOL / 5, small enough not to eat the bar the device is held to.

Teeth: the comparator fed the oracle's own gradients in the device's place passes; with the rows of the flip-touched
Gaussians 3 % wrong, the assertions that existed before the masked leg still pass (the hole the leg closes, kept on
record) and the whole comparator fails, as it does at 1e-4.
"""
import functools

import numpy as np
import pytest

from tests import edge_cases as E
from tests.helpers import rel_l2, run_oracle, scene_inputs, upstream
from tests.test_gpu_parity import (FLIP_PIXEL_CAP, GRAD_CLEAN_TOL, GRADS, assert_backward_bars, backward_figures,
                                   flip_candidates, touched_gaussians)

LINEARITY_TOL = 1e-6
LONG_TILES = "long_tiles_60000_96x64"


@functools.lru_cache(maxsize=None)
def _scene(name):
    """(oracle run with its flip census attached, dL_dcolor, dL_dinvdepth, image width)."""
    if name == "edge_rotations":
        full, dc, di = E.build("rotations")
        inp = E.rasterizer_inputs(full)
    else:
        n, W, H, deg, seed, up = {LONG_TILES: (60_000, 96, 64, 1, 23, 5), "unsat_3000_200x136": (3000, 200, 136, 3, 2, 2),
                                  "cfg1_10000_256x256": (10_000, 256, 256, 0, 0, 0)}[name]
        inp = scene_inputs(n, W, H, sh_degree=deg, seed=seed)
        dc, di = upstream(W, H, up)
    run = run_oracle(inp)[3]
    run.flip_mask = flip_candidates(run)
    run.flip_touched = touched_gaussians(run.flip_mask, run.image_state()[1], run.point_list(), run.ranges(),
                                         inp["image_width"], run.P)
    return run, dc, di


@functools.lru_cache(maxsize=None)
def _oracle_as_device(name):
    """The oracle's own gradients in the device's place: the plain backward and the direct backward of the upstream
    gradient zeroed on the flip candidates."""
    run, dc, di = _scene(name)
    keep = (~run.flip_mask).astype(np.float32)[None]
    return run.backward(dc, di), run.backward(dc * keep, di * keep)


@pytest.mark.parametrize("name", [LONG_TILES, "unsat_3000_200x136", "cfg1_10000_256x256", "edge_rotations"])
def test_masked_oracle_gradient_is_the_difference(name):
    """g - g_flip (float64) against the oracle's direct backward of the masked upstream gradient.  Measured maxima over
    the six gradients: long tiles 1.1e-7 (scales; 10 candidates of 6,144 pixels), the 3000-Gaussian scene 3.9e-7
    (rotations; 1 candidate), cfg 1 4.0e-8 (rotations; 6 candidates), edge `rotations` 1.7e-7 (scales; 1 candidate)."""
    run, dc, di = _scene(name)
    g, direct = _oracle_as_device(name)
    m = run.flip_mask.astype(np.float32)[None]
    gf = run.backward(dc * m, di * m)
    assert run.flip_mask.mean() <= FLIP_PIXEL_CAP
    err = {k: rel_l2(np.asarray(g[k], np.float64) - np.asarray(gf[k], np.float64), direct[k]) for k in GRADS}
    print(name, int(run.flip_mask.sum()), "flip pixels", err)
    for k, e in err.items():
        assert e <= LINEARITY_TOL, (k, e)


def _perturbed(grads, touched, factor):
    out = {k: np.array(grads[k], copy=True) for k in GRADS}
    for k in GRADS:
        out[k][touched] *= np.float32(factor)
    return out


def test_scene_has_flip_candidates_in_long_tiles():
    """The teeth below bite only if the scene has what the masked leg is for: a few candidate pixels whose walks mark
    thousands of Gaussians as touched."""
    run, _, _ = _scene(LONG_TILES)
    assert 1 <= run.flip_mask.sum() <= FLIP_PIXEL_CAP * run.flip_mask.size
    assert run.flip_touched.sum() >= 5000


def test_comparator_passes_the_oracle_itself():
    run, dc, di = _scene(LONG_TILES)
    g, gm = _oracle_as_device(LONG_TILES)
    rec, _ = backward_figures(g, gm, run, dc, di)
    assert rec["masked_leg"]
    assert_backward_bars(rec)
    for k in GRADS:
        assert rec[k]["rel_l2"] == 0.0 and rec[k]["rel_l2_masked"] <= LINEARITY_TOL, (k, rec[k])


def test_three_percent_on_the_touched_rows_passes_the_old_bars_and_fails_the_masked_leg():
    """The hole: 3 % on every gradient row of the touched Gaussians is 2.2e-2 / 2.2e-2 / 2.1e-2 relative L2 in
    means3D / scales / shs, under the derived bars of 7.1e-2 / 5.5e-2 / 7.9e-2, and leaves the clean set untouched."""
    run, dc, di = _scene(LONG_TILES)
    g, gm = _oracle_as_device(LONG_TILES)
    t = run.flip_touched
    rec, _ = backward_figures(_perturbed(g, t, 1.03), _perturbed(gm, t, 1.03), run, dc, di)
    assert_backward_bars(rec, masked_leg=False)  # every assertion from before the masked leg passes
    for k in GRADS:
        assert rec[k]["rel_l2"] > 1e-3, (k, rec[k])  # ... on gradients that are wrong at the 1e-2 level
    with pytest.raises(AssertionError):
        assert_backward_bars(rec)
    for k in GRADS:
        assert rec[k]["rel_l2_masked"] > 1e-3 > GRAD_CLEAN_TOL, (k, rec[k])


def test_one_in_ten_thousand_on_the_touched_rows_fails():
    run, dc, di = _scene(LONG_TILES)
    g, gm = _oracle_as_device(LONG_TILES)
    t = run.flip_touched
    rec, _ = backward_figures(_perturbed(g, t, 1.0 + 1e-4), _perturbed(gm, t, 1.0 + 1e-4), run, dc, di)
    with pytest.raises(AssertionError):
        assert_backward_bars(rec)
    for k in GRADS:
        assert rec[k]["rel_l2_masked"] > GRAD_CLEAN_TOL, (k, rec[k])


def test_missing_masked_backward_is_an_error():
    """A caller that has flip candidates and did not run the masked backward fails; it is not skipped."""
    run, dc, di = _scene(LONG_TILES)
    g, _ = _oracle_as_device(LONG_TILES)
    rec, _ = backward_figures(g, None, run, dc, di)
    with pytest.raises(AssertionError):
        assert_backward_bars(rec)
