"""Scenes, upstream gradients and oracle ground truth of the depth-distortion tests (gsr_forward_distortion /
gsr_backward_distortion).

Per pixel, over the pairs the colour forward composited, with w_i = alpha_i T_i and a per-Gaussian depth t_i:
    D(pix) = sum_i sum_j w_i w_j |t_i - t_j| = 2 sum_i w_i (t_i A_<i - M_<i)        (t non-decreasing along the walk)
    c_i = dD/dw_i = 2 [t_i (A_<i - A_>i) - M_<i + M_>i],    dD/dt_i = 2 w_i (A_<i - A_>i).

The truth comes from the CPU oracle alone.  tests/contrib_cases.py's pixel_weights_of_gaussians gives the oracle's own
w_.(pix), exactly 0 for a pair not taken; the contributors are ordered by the tile's point_list and t comes from the
oracle's view depths.  D, c and dD/dt are formed in float64.  The gradient through the weights is the gradient of
sum_i c_i w_i(pix) with c frozen: what an oracle run returns with colors_precomp[:, ch] = c_.(pix), background 0 and a
backward whose dL_dcolor is g(pix) at that pixel in that channel -- three pixels per call, summed in float64.  The direct
depth part is analytic: z = means3D . V[:3,2] + V[3,2], so sum_pix g dD/dt_i dt/dz V[:3,2] is added to means3D.

The same formulas are also evaluated in numpy float32 in two association orders -- "prefix": the prefix sums taken
directly, "suffix": the prefix sums as total - suffix - w_i, as a reverse walk has them -- and carried through the same
oracle calls: their errors against the float64 truth are what the distortion's own cancellation costs in fp32, and set
the tests' bars (bar()).  Nothing here reads the device's output.

Scenes: those of tests/absgrad_cases.py with the stored inputs of tests/golden/absgrad.npz.  Scene B takes about
11,000 oracle calls per map and order, so the tests read the truths from tests/golden/distortion.npz
(tests/golden/make_golden_distortion.py); a host test recomputes scene A and compares.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import absgrad_cases as AC
from tests import contrib_cases as CC
from tests.helpers import load_golden, run_oracle

f32, f64 = np.float32, np.float64
SCENES = ("A", "A2", "B")
MAPS = ("z", "ndc")
NEAR, FAR = 0.5, 20.0  # the "ndc" map's planes: the scenes' view depths lie between them
GEOMETRY = ("means3D", "means2D", "opacities", "scales", "rotations")
ORDERS = ("prefix", "suffix")
G_SEED = 307
RESTATEMENT_MARGIN = 4.0  # the margin the SSIM tests give their restatements


def scene(name):
    """The scene's inputs with the absgrad fixture's stored inputs."""
    return CC.scene(name)


@functools.lru_cache(maxsize=None)
def upstream(name):
    """g = dL/dD: a seeded standard-normal (1,H,W) float32."""
    _, W, H, seed = AC.SCENES[name][:4]
    return np.random.default_rng(G_SEED + seed).standard_normal((1, H, W)).astype(f32)


def depth_map(which, z, dtype=f64):
    """(t, dt/dz) of a map at view depths z, every operation in dtype."""
    z = np.asarray(z, dtype)
    z = np.where(z > 0, z, dtype(1))  # (a culled Gaussian's depth is not set: it has no pair)
    if which == "z":
        return z, np.ones_like(z)
    near, far = dtype(NEAR), dtype(FAR)
    return far / (far - near) * (dtype(1) - near / z), far * near / ((far - near) * z * z)


@functools.lru_cache(maxsize=None)
def pixel_lists(name):
    """Per pixel (row-major): (Gaussian ids of its contributors front to back, their oracle weights w float32)."""
    n, W, H = AC.SCENES[name][:3]
    run = CC.oracle_run(name)
    pl, rg = run.point_list().astype(np.int64), run.ranges()
    gx = (W + 15) // 16
    out = [None] * (W * H)
    for (y, x), w in CC.pixel_weights_of_gaussians(name):
        assert not np.any(w < 0)
        lo, hi = rg[(y // 16) * gx + x // 16]
        ids = pl[lo:hi]
        assert ids.size == np.unique(ids).size and np.count_nonzero(w) == np.count_nonzero(w[ids])
        ids = ids[w[ids] > 0]
        out[y * W + x] = (ids, w[ids].copy())
    return out


def pixel_terms(w, t, order=None):
    """(D, c (k,), dD/dt (k,)) of one pixel from its contributors' weights and depths, front to back.  order None:
    float64; "prefix" / "suffix": float32 throughout, the prefix sums taken directly or as total - suffix - own."""
    dt = f64 if order is None else f32
    w, t = w.astype(dt), t.astype(dt)
    wt = w * t
    two = dt(2)
    zero = np.zeros(min(1, w.size), dt)
    A_inc, M_inc = np.cumsum(w), np.cumsum(wt)  # front to back, in dt (empty for a pixel without contributors)
    if order == "suffix":
        A_gt = np.concatenate([np.cumsum(w[::-1])[::-1][1:], zero])  # back to front
        M_gt = np.concatenate([np.cumsum(wt[::-1])[::-1][1:], zero])
        A_lt, M_lt = (A_inc[-1:] - A_gt) - w, (M_inc[-1:] - M_gt) - wt
    else:
        A_lt, M_lt = np.concatenate([zero, A_inc[:-1]]), np.concatenate([zero, M_inc[:-1]])
        A_gt, M_gt = A_inc[-1:] - A_inc, M_inc[-1:] - M_inc
    terms = w * (t * A_lt - M_lt)
    D = two * (np.cumsum(terms)[-1] if w.size else dt(0))
    dA = A_lt - A_gt
    return D, two * (t * dA - M_lt + M_gt), two * w * dA


def explicit_double_sum(w, t):
    """sum_i sum_j w_i w_j |t_i - t_j| in float64: the definition."""
    w, t = w.astype(f64), t.astype(f64)
    return float((w[:, None] * w[None, :] * np.abs(t[:, None] - t[None, :])).sum())


def coefficients(name, which, order=None):
    """(D (H,W), C (H*W, P) float32 = c_.(pix), zero for a pair not taken, depth term (P,) = sum_pix g dD/dt_i) in
    float64 (order None) or in a float32 restatement."""
    n, W, H = AC.SCENES[name][:3]
    dt = f64 if order is None else f32
    z = CC.oracle_run(name).geom()["depths"]
    t = depth_map(which, z, dt)[0]
    g = upstream(name)[0].astype(dt)
    D = np.zeros((H, W), dt)
    C = np.zeros((H * W, n), f32)
    dterm = np.zeros(n, dt)
    for pix, (ids, w) in enumerate(pixel_lists(name)):
        d, c, ddt = pixel_terms(w, t[ids], order)
        D[pix // W, pix % W] = d
        C[pix, ids] = c.astype(f32)
        dterm[ids] += g[pix // W, pix % W] * ddt
    return D, C, dterm


def weight_gradient(name, C):
    """Float64 geometry gradients of sum_pix g(pix) sum_i C[pix, i] w_i(pix) with C frozen: one oracle forward and
    backward per three pixels (one per colour channel).  (The runs' decisions are those of CC.oracle_run: they do not
    depend on the colours, so its flip census is theirs.)"""
    n, W, H = AC.SCENES[name][:3]
    inp = dict(scene(name), bg=np.zeros(3, f32))
    g = upstream(name)[0]
    out = {k: 0 for k in GEOMETRY}
    for p0 in range(0, W * H, 3):
        col = np.zeros((n, 3), f32)
        dc = np.zeros((3, H, W), f32)
        for ch, pix in enumerate(range(p0, min(p0 + 3, W * H))):
            col[:, ch] = C[pix]
            dc[ch, pix // W, pix % W] = g[pix // W, pix % W]
        if not col.any():
            continue
        run = run_oracle(inp, colors_precomp=col)[3]
        b = run.backward(dc, None)
        for k in GEOMETRY:
            out[k] = out[k] + b[k].astype(f64)
    return out


def gradients(name, which, order=None):
    """(D, {GEOMETRY: float64 gradient of sum_pix g D}, depth term (P,) float64, flip candidates): through the weights
    by the oracle, through the depths analytically."""
    D, C, dterm = coefficients(name, which, order)
    grads = weight_gradient(name, C)
    inp = scene(name)
    z = CC.oracle_run(name).geom()["depths"]
    dz = dterm.astype(f64) * depth_map(which, z, f64 if order is None else f32)[1].astype(f64)
    grads["means3D"] = grads["means3D"] + dz[:, None] * inp["viewmatrix"].astype(f64)[:3, 2][None, :]
    return D.astype(f64), grads, dz, CC.flip_candidates(name)


def fwd_error(D, truth):
    """max over the pixels of |D - truth| / max(1, |truth|)."""
    return float((np.abs(np.asarray(D, f64) - truth) / np.maximum(1.0, np.abs(truth))).max())


def truth(name, which):
    """Everything the fixture stores of one (scene, map): the float64 truth, and the absolute errors of the two
    float32 restatements against it (forward: fwd_error; gradients: the L2 norm of the difference, per tensor)."""
    D, grads, dz, flips = gradients(name, which)
    out = {"D": D, "dz": dz, "flip_candidates": np.int64(flips), **grads}
    for order in ORDERS:
        D32, g32, _, _ = gradients(name, which, order)
        out[f"err_{order}_D"] = f64(fwd_error(D32, D))
        for k in GEOMETRY:
            out[f"err_{order}_{k}"] = f64(np.linalg.norm(g32[k] - grads[k]))
    return out


@functools.lru_cache(maxsize=None)
def fixture_truth(name, which):
    z = load_golden("distortion")
    pre = f"{name}_{which}_"
    return {k[len(pre):]: v for k, v in z.items() if k.startswith(pre)}


def restatement_error(t, key):
    """The worse of the two float32 restatements' errors of one quantity ("D" or a GEOMETRY tensor)."""
    return max(float(t[f"err_{order}_{key}"]) for order in ORDERS)


def bar(t, key, suite_bar, norm=None):
    """The bar of one comparison: the larger of the suite's own bar (the oracle part of the truth carries the suite's
    fp32 error) and RESTATEMENT_MARGIN x the worse float32 restatement's error -- for a gradient the restatement's
    absolute error over `norm`, the L2 norm of the truth the test compares against (a joint call's is larger)."""
    e = restatement_error(t, key)
    return max(suite_bar, RESTATEMENT_MARGIN * (e if norm is None else e / norm))
