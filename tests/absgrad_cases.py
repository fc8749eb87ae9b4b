"""Scenes and oracle ground truth of the absolute screen-space gradient (AbsGS) tests.

abs_i = (sum_pix |m_x(i,pix)|, sum_pix |m_y(i,pix)|), with m(i,pix) what pixel pix adds to dL/dmeans2D[i][:2].  The
oracle has no such output, but its backward can be called repeatedly on one forward: with the upstream gradients
masked to a single pixel its means2D[:, :2] IS that pixel's m(., pix).  The truth is the float64 sum of the absolute
values of those per-pixel calls; their signed sum reproduces the oracle's full backward (recorded as
`signed_residual`), which checks the decomposition itself.

With an alpha gradient a and a background image B the oracle has no direct answer either; the per-pixel m is composed
by linearity as tests/test_alpha_background.py composes the full gradient: run A (background 0, backward of (g, di))
plus run B (colours 0, background 1, so colour channel 0 is T_final; backward of (tau, 0, 0)) with
tau = sum_c B_c g_c - a -- pixel by pixel, before the absolute value is taken.

Used by tests/test_absgrad.py and by the generator of its fixture, tests/golden/make_golden_absgrad.py (scene B's
truth takes ~20 s of oracle calls, so the tests read it from tests/golden/absgrad.npz).
"""
from __future__ import annotations

import hashlib

import numpy as np

from tests.helpers import run_oracle, scene_inputs, upstream

f32 = np.float32
FLIP_MARGIN = 1.0  # tests/test_gpu_parity.py: oracle threshold margin below which a pixel is a flip candidate

# name: (n, W, H, seed, scale factor, stress_fraction)
SCENES = {
    "A": (600, 40, 24, 3, 1.0, 0.0),    # 3x2 tiles, both edges partial; longest tile > 64 and > 32 batches
    "A2": (600, 40, 24, 3, 2.5, 0.0),   # the same with scales x 2.5: most pixels saturate
    "B": (60, 136, 120, 5, 1.0, 0.1),   # 9x8 tiles, both edges partial; Gaussians with > 64 instances (big_reduce)
}
EXT_SEED = 11  # scene A's alpha gradient and background image (the ABS x EXT form)


# inputs the fixture stores instead of regenerating them (tests/helpers.py REF_STORED_INPUTS: anything formed with more
# than a seeded randn and one rounding can round differently on another CPU's vector units)
STORED_INPUTS = ("scales", "rotations", "opacities", "viewmatrix", "projmatrix", "campos")


def scene(name, fixture=None):
    """(inputs, dL_dcolor (3,H,W), dL_dinvdepth (1,H,W)) of one scene; with the fixture (load_golden("absgrad")) the
    STORED_INPUTS are the generator's own."""
    n, W, H, seed, scale, stress = SCENES[name]
    inp = scene_inputs(n, W, H, sh_degree=3, seed=seed, stress_fraction=stress)
    if scale != 1.0:
        inp = dict(inp, scales=(inp["scales"] * f32(scale)).astype(f32))
    if fixture is not None:
        inp = dict(inp, **{k: fixture[f"{name}_input_{k}"] for k in STORED_INPUTS})
    dc, di = upstream(W, H, seed + 1)
    return inp, dc, di


def ext_inputs():
    """(dL_dalpha (1,H,W), background image (3,H,W) in [0, 1]) of scene A's ABS x EXT case."""
    _, W, H = SCENES["A"][:3]
    rng = np.random.default_rng(EXT_SEED)
    return rng.standard_normal((1, H, W)).astype(f32), rng.random((3, H, W), dtype=f32)


def input_hash(name) -> str:
    """SHA-256 of the regenerated inputs (the plain seeded draws; the others are stored)."""
    inp, dc, di = scene(name)
    h = hashlib.sha256()
    for a in (inp["means3D"], inp["shs"], dc, di) + (ext_inputs() if name == "A" else ()):
        h.update(np.ascontiguousarray(a, f32).tobytes())
    return h.hexdigest()


def census(run) -> dict:
    """What a scene must exercise, from the oracle's forward."""
    ft, nc = run.image_state()
    rg = run.ranges()
    tiles = run.geom()["tiles_touched"]
    return dict(instances=int(run.num_rendered), longest_tile=int((rg[:, 1] - rg[:, 0]).max()),
                saturated=int((ft < 0.01).sum()), above_half=int((ft > 0.5).sum()), untouched=int((nc == 0).sum()),
                flip_candidates=int((run.threshold_margin() < FLIP_MARGIN).sum()),
                big_gaussians=int((tiles > 64).sum()), most_instances=int(tiles.max()))


def per_pixel_abs(runs_and_grads, P, W, H):
    """Float64 (abs (P,2), signed (P,2)) over the pixels.  runs_and_grads: [(oracle run, dL_dcolor (3,H,W),
    dL_dinvdepth (1,H,W) or None)], whose single-pixel backwards are added per pixel before the absolute value."""
    tot_abs = np.zeros((P, 2), np.float64)
    tot = np.zeros((P, 2), np.float64)
    for y in range(H):
        for x in range(W):
            m = np.zeros((P, 2), np.float64)
            for run, g, d in runs_and_grads:
                g1 = np.zeros_like(g)
                g1[:, y, x] = g[:, y, x]
                d1 = None
                if d is not None:
                    d1 = np.zeros_like(d)
                    d1[:, y, x] = d[:, y, x]
                if not g1.any() and (d1 is None or not d1.any()):
                    continue
                m += run.backward(g1, d1)["means2D"][:, :2]
            tot_abs += np.abs(m)
            tot += m
    return tot_abs, tot


def truth(name, with_invdepth=True, fixture=None):
    """(abs, signed, the oracle's full-backward means2D[:, :2], the oracle run) of a scene's plain case."""
    inp, dc, di = scene(name, fixture)
    n, W, H = SCENES[name][:3]
    run = run_oracle(inp)[3]
    d = di if with_invdepth else None
    a, s = per_pixel_abs([(run, dc, d)], n, W, H)
    return a, s, run.backward(dc, d)["means2D"][:, :2].astype(np.float64), run


def truth_ext(fixture=None):
    """(abs, signed) of scene A with the alpha gradient and the background image of ext_inputs()."""
    inp, dc, di = scene("A", fixture)
    n, W, H = SCENES["A"][:3]
    da, image = ext_inputs()
    run_a = run_oracle(dict(inp, bg=np.zeros(3, f32)))[3]
    run_b = run_oracle(dict(inp, bg=np.ones(3, f32)), colors_precomp=np.zeros((n, 3), f32))[3]
    tau = ((image.astype(np.float64) * dc.astype(np.float64)).sum(0) - da[0].astype(np.float64)).astype(f32)
    t3 = np.zeros((3, H, W), f32)
    t3[0] = tau
    return per_pixel_abs([(run_a, dc, di), (run_b, t3, None)], n, W, H)
