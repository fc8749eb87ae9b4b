"""Scenes, weight images and oracle ground truth of the contribution-statistics tests (gsr_contributions).

Per Gaussian i, over the pixels whose weight m(pix) is > 0 (every pixel without a weight image) and that the colour
forward composited Gaussian i into: count[i] the number of those pixels, wsum[i] the sum and wmax[i] the max of
v = m(pix) * w_i(pix), w_i = alpha_i T_i.

The truth comes from the CPU oracle alone.  One forward with precomputed colours; its backward's colour gradient is
dL_dcolors[i][c] = sum_pix w_i(pix) g_c(pix), so an upstream gradient with a single 1 at one pixel of channel 0, at
another pixel of channel 1 and at a third of channel 2 yields w_.(pix) of three pixels per call, in the oracle's own
arithmetic: exactly 0 for a pair that does not contribute and > 0 for one that does (alpha >= 1/255, T > 1e-4).  From
these, in float64: count = #{m > 0 and w > 0}, wsum = sum f32(m) * w, wmax = max f32(m) * w.

Scenes: those of tests/absgrad_cases.py with the stored inputs of tests/golden/absgrad.npz.  Scene B takes about 5,400
oracle calls, so the tests read the truths from tests/golden/contrib.npz (tests/golden/make_golden_contrib.py); the
host test recomputes scene A and compares.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import absgrad_cases as AC
from tests.helpers import load_golden, run_oracle

f32 = np.float32
SCENES = ("A", "A2", "B")
WEIGHT_SEED = 211
KINDS = ("count", "wsum", "wmax")


@functools.lru_cache(maxsize=None)
def scene(name):
    """The scene's inputs with the absgrad fixture's stored inputs."""
    return AC.scene(name, load_golden("absgrad"))[0]


@functools.lru_cache(maxsize=None)
def weights(name):
    """The scene's weight image (H,W) float32: uniform in [0, 1), about a quarter of the pixels exactly 0 and about 3 %
    negative (both left out of every statistic).  Plain seeded draws and comparisons: the same on every CPU."""
    _, W, H, seed = AC.SCENES[name][:4]
    rng = np.random.default_rng(WEIGHT_SEED + seed)
    m = rng.random((H, W), dtype=f32)
    pick = rng.random((H, W), dtype=f32)
    m[pick < f32(0.25)] = f32(0.0)
    m[pick > f32(0.97)] *= f32(-1.0)
    return m


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    """The oracle's forward of the scene with (zero) precomputed colours over a zero background."""
    inp = scene(name)
    n = AC.SCENES[name][0]
    return run_oracle(dict(inp, bg=np.zeros(3, f32)), colors_precomp=np.zeros((n, 3), f32))[3]


def flip_candidates(name) -> int:
    """Pixels of the scene with a threshold-flip candidate (tests/test_gpu_parity.py FLIP_MARGIN): the tests assert 0."""
    return int((oracle_run(name).threshold_margin() < AC.FLIP_MARGIN).sum())


def pixel_weights_of_gaussians(name):
    """Yields (pixel index (y, x), w (P,) float32 = the oracle's w_.(pix)) for every pixel, three per oracle call."""
    n, W, H = AC.SCENES[name][:3]
    run = oracle_run(name)
    pix = [(y, x) for y in range(H) for x in range(W)]
    for p0 in range(0, len(pix), 3):
        g = np.zeros((3, H, W), f32)
        group = pix[p0:p0 + 3]
        for c, (y, x) in enumerate(group):
            g[c, y, x] = f32(1.0)
        col = run.backward(g, None)["colors"]
        for c, yx in enumerate(group):
            yield yx, col[:, c]


def truth(name):
    """{"count", "wsum", "wmax"} without a weight image and {"m_count", "m_wsum", "m_wmax"} under weights(name): count
    int64, the others float64, (P,) each."""
    n = AC.SCENES[name][0]
    m = weights(name)
    out = dict(count=np.zeros(n, np.int64), wsum=np.zeros(n, np.float64), wmax=np.zeros(n, np.float64),
               m_count=np.zeros(n, np.int64), m_wsum=np.zeros(n, np.float64), m_wmax=np.zeros(n, np.float64))
    for (y, x), w in pixel_weights_of_gaussians(name):
        assert not np.any(w < 0)
        w64 = w.astype(np.float64)
        out["count"] += w > 0
        out["wsum"] += w64
        np.maximum(out["wmax"], w64, out=out["wmax"])
        if m[y, x] > 0:
            v = np.float64(m[y, x]) * w64
            out["m_count"] += w > 0
            out["m_wsum"] += v
            np.maximum(out["m_wmax"], v, out=out["m_wmax"])
    return out


@functools.lru_cache(maxsize=None)
def fixture_truth(name, weighted: bool):
    """dict(count, wsum, wmax) of the scene from tests/golden/contrib.npz, with or without the weight image."""
    z = load_golden("contrib")
    pre = "m_" if weighted else ""
    return {k: z[f"{name}_{pre}{k}"] for k in KINDS}
