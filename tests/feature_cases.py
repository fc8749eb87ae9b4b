"""Scenes, inputs and oracle ground truth of the feature-channel tests (gsr_forward_features / gsr_backward_features).

The oracle composites three colour channels.  A feature image is linear in the features and shares the colour's
weights, so the truth comes from the oracle alone: for channels [c0, c0 + 3) run it with colors_precomp = that chunk
(background 0, the last chunk zero-padded); its colour IS the feature image of those channels, its
backward(dF_chunk, 0) gives `colors` = dL_dfeatures of the chunk, and the geometry gradients of the chunks add up (in
float64).  A joint call adds the SH colour run's backward(dL_dcolor, dL_dinvdepth); an alpha gradient and a background
image are composed the way tests/test_alpha_background.py composes them (run A: background 0; run B: colours 0,
background 1, backward of (tau, 0, 0) with tau = sum_c B_c g_c - a).

Scenes: those of tests/absgrad_cases.py with the fixture's stored inputs (no threshold-flip candidate in any of them,
with precomputed colours too: asserted from the oracle by every test that uses a truth).  Features and dL/dF are
standard-normal draws of the full 64 channels per scene; C channels are the first C of them, so a chunk's oracle run
is shared by every C that contains it whole.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import absgrad_cases as AC
from tests.helpers import load_golden, run_oracle

f32 = np.float32
MAX_C = 64
GEOMETRY = ("means3D", "means2D", "opacities", "scales", "rotations")
FEATURE_SEED = 101


@functools.lru_cache(maxsize=None)
def scene(name):
    """(inputs, dL_dcolor, dL_dinvdepth) with the absgrad fixture's stored inputs."""
    return AC.scene(name, load_golden("absgrad"))


@functools.lru_cache(maxsize=None)
def draws(name):
    """(features (P,64), dL_dF (64,H,W)): seeded standard-normal draws, negative values included."""
    n, W, H, seed = AC.SCENES[name][:4]
    rng = np.random.default_rng(FEATURE_SEED + seed)
    return rng.standard_normal((n, MAX_C)).astype(f32), rng.standard_normal((MAX_C, H, W)).astype(f32)


def inputs(name, C):
    f, dF = draws(name)
    return np.ascontiguousarray(f[:, :C]), np.ascontiguousarray(dF[:C])


def _pad3(a, axis):
    """Zero-pad a chunk of 1..3 channels to 3 along axis."""
    pad = [(0, 0)] * a.ndim
    pad[axis] = (0, 3 - a.shape[axis])
    return np.pad(a, pad)


def chunk_truth(inp, f_chunk, dF_chunk=None):
    """One oracle call for up to three channels: (image (w,H,W), flip candidates, backward dict or None)."""
    w = f_chunk.shape[1]
    color, _, _, run = run_oracle(dict(inp, bg=np.zeros(3, f32)), colors_precomp=_pad3(f_chunk, 1))
    flips = int((run.threshold_margin() < AC.FLIP_MARGIN).sum())
    g = None
    if dF_chunk is not None:
        g = run.backward(_pad3(dF_chunk, 0), None)
    return color[:w], flips, g


@functools.lru_cache(maxsize=None)
def _chunk(name, c0, w):
    f, dF = draws(name)
    return chunk_truth(scene(name)[0], f[:, c0:c0 + w], dF[c0:c0 + w])


@functools.lru_cache(maxsize=None)
def truth(name, C):
    """dict(image (C,H,W) f32, features (P,C) f32, means3D.. float64 sums over the chunks, flip_candidates)."""
    n = AC.SCENES[name][0]
    out = dict(image=[], features=np.zeros((n, C), f32), flip_candidates=0)
    for c0 in range(0, C, 3):
        w = min(3, C - c0)
        img, flips, g = _chunk(name, c0, w)
        out["image"].append(img)
        out["features"][:, c0:c0 + w] = g["colors"][:, :w]
        out["flip_candidates"] += flips
        for k in GEOMETRY:
            out[k] = out.get(k, 0) + g[k].astype(np.float64)
    out["image"] = np.concatenate(out["image"], 0)
    return out


@functools.lru_cache(maxsize=None)
def joint_truth(name, C, ext=False):
    """The joint call's truth: SH colour + inverse depth + features; ext (scene A): also absgrad_cases.ext_inputs()'
    alpha gradient and background image, composed as in tests/test_alpha_background.py.  Adds "shs"."""
    inp, dc, di = scene(name)
    n, W, H = AC.SCENES[name][:3]
    t = dict(truth(name, C))
    run_a = run_oracle(dict(inp, bg=np.zeros(3, f32)))[3]
    t["flip_candidates"] += int((run_a.threshold_margin() < AC.FLIP_MARGIN).sum())
    a = run_a.backward(dc, di)
    for k in GEOMETRY:
        t[k] = t[k] + a[k].astype(np.float64)
    t["shs"] = a["shs"].astype(np.float64)
    if ext:
        da, image = AC.ext_inputs()
        run_b = run_oracle(dict(inp, bg=np.ones(3, f32)), colors_precomp=np.zeros((n, 3), f32))[3]
        tau = ((image.astype(np.float64) * dc.astype(np.float64)).sum(0) - da[0].astype(np.float64)).astype(f32)
        t3 = np.zeros((3, H, W), f32)
        t3[0] = tau
        b = run_b.backward(t3, None)
        for k in GEOMETRY:
            t[k] = t[k] + b[k].astype(np.float64)
    return t
