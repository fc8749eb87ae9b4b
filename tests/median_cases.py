"""Scenes, upstream gradients and oracle ground truth of the median-depth tests (gsr_forward_median /
gsr_backward_median), and the float64 restatement of the normal consistency on the blended surface.

Per pixel, over the pairs the colour forward composited, front to back: the median is the last contributor whose
incoming transmittance exceeds 1/2 (2DGS's rule), the last contributor at all on a pixel that never becomes half
opaque; median_depth is that Gaussian's view depth, median_index its id; 0 and -1 where no Gaussian reaches.

The truth comes from the CPU oracle alone, never from the device.  tests/distortion_cases.py's pixel_lists gives each
pixel's contributors front to back with the oracle's own weights w_i = alpha_i T_i; the incoming transmittance of
contributor i is 1 - sum_(j<i) w_j in float64; the depth is the oracle's geom()["depths"] of the selected Gaussian.

Threshold condition.  The device carries T as a float32 product, so a pixel whose incoming T passes within
MEDIAN_MARGIN of 0.5 at some contributor may legitimately select a neighbour: such a pixel is a *candidate*.  The
margin of a scene is derived from its longest contributor list (margin()).  On a candidate the device's index must
still be one of the two contributors adjacent to the crossing ("adjacent" below); every other pixel is compared in
full.  The upstream gradient of the backward tests is zero on the candidates (upstream()): there the gradient's
destination is as ambiguous as the selection.

The gradient: the selection is piecewise constant, so dL/dz_i = sum over the pixels whose median is i of g(pix), and
z = means3D . V[:3,2] + V[3,2] carries it to means3D (and to column 2 of the view matrix); nothing else gets any.
The same sum is restated in numpy float32 over the pixels in another order (restated()); its error against the
float64 truth is what the sum costs in fp32 and sets the tests' bars (bar()).

Scenes: those of tests/absgrad_cases.py with the stored inputs of tests/golden/absgrad.npz.  Scene B takes about
5,400 oracle calls, so the tests read the truths from tests/golden/median.npz (tests/golden/make_golden_median.py); a
host test recomputes scene A and compares.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from tests import absgrad_cases as AC
from tests import contrib_cases as CC
from tests import distortion_cases as DC
from tests import normal_cases as NC
from tests.helpers import load_golden

f32, f64 = np.float32, np.float64
SCENES = ("A", "A2", "B")
G_SEED = 911
RESTATEMENT_MARGIN = 4.0  # as tests/distortion_cases.py
# The device's T at contributor i is a float32 product of i factors (1 - alpha_j).  A factor carries four roundings of
# 2^-24 relative each -- the exponential, the product with the opacity, the subtraction from 1, the multiplication into
# T -- so about 2^-22 relative, and T near 0.5 after L factors about 0.5 L 2^-22 = L 2^-23 absolute.  (The truth's own
# error is far below: a float64 sum of float32 weights, at most 2^-24.)  MARGIN_FACTOR covers the exponentials of the
# device and the oracle differing by more than one rounding.
MARGIN_FACTOR = 4.0
MAX_CANDIDATE_FRACTION = 1e-3  # of a scene's pixels


def scene(name):
    """The scene's inputs with the absgrad fixture's stored inputs."""
    return CC.scene(name)


def margin(longest: int) -> float:
    """MEDIAN_MARGIN of a scene whose longest contributor list has `longest` entries."""
    return float(longest) * 2.0 ** -23 * MARGIN_FACTOR


def pixel_median(w):
    """(position k of the median in the pixel's contributor list or -1, incoming transmittances (n,) float64) from the
    contributors' oracle weights, front to back."""
    if w.size == 0:
        return -1, np.zeros(0, f64)
    t_in = 1.0 - np.concatenate([[0.0], np.cumsum(w.astype(f64))[:-1]])
    return int(np.nonzero(t_in > 0.5)[0][-1]), t_in  # (t_in[0] = 1: never empty)


@functools.lru_cache(maxsize=None)
def truth(name):
    """Everything the fixture stores of one scene, from the oracle: index (H,W) int32, depth (H,W) float32 (the
    oracle's view depth of that Gaussian, bit for bit; 0 and -1 where no Gaussian reaches), z (P,) float32 (the oracle's
    view depth of every Gaussian), candidate (H,W) bool,
    adjacent (H,W,2) int32 (the two contributors either of which a candidate pixel may select; the index twice
    elsewhere), last (H,W) bool (the transmittance reaching the pixel's last contributor still exceeds 1/2 -- it never
    fell to 1/2 along the walk -- so the median is that last contributor), longest (the longest contributor list), margin, closest (the smallest distance of an
    incoming transmittance to 0.5), max_distinct (the most distinct medians in one tile), flip_candidates, and the
    gradient truth under upstream(): dz (P,) and means3D (P,3) float64, err_means3D / err_dz the float32 restatement's
    absolute errors (L2)."""
    n, W, H = AC.SCENES[name][:3]
    lists = DC.pixel_lists(name)
    z = CC.oracle_run(name).geom()["depths"].astype(f32)
    longest = max(ids.size for ids, _ in lists)
    m = margin(longest)
    index = np.full((H, W), -1, np.int32)
    depth = np.zeros((H, W), f32)
    cand = np.zeros((H, W), bool)
    adj = np.full((H, W, 2), -1, np.int32)
    last = np.zeros((H, W), bool)
    closest = np.inf
    for pix, (ids, w) in enumerate(lists):
        y, x = divmod(pix, W)
        k, t_in = pixel_median(w)
        if k < 0:
            continue
        index[y, x] = ids[k]
        depth[y, x] = z[ids[k]]
        adj[y, x] = ids[k]
        last[y, x] = k == ids.size - 1
        dist = np.abs(t_in - 0.5)
        closest = min(closest, float(dist.min()))
        near = np.nonzero(dist <= m)[0]
        if near.size:
            # incoming T of contributor i within the margin of 0.5: the device may decide "T > 0.5" at i either way, so
            # its median is contributor i or the one before it.  One i at most: a contributor's alpha is at least 1/255,
            # so its neighbours' incoming T lie 0.5 / 255 or more away; and i > 0, the first one's being 1.
            cand[y, x] = True
            assert near.size == 1 and near[0] > 0
            i = int(near[0])
            adj[y, x] = (ids[i - 1], ids[i])
            assert index[y, x] in adj[y, x]
    gx = (W + 15) // 16
    per_tile = {}
    for y in range(H):
        for x in range(W):
            if index[y, x] >= 0:
                per_tile.setdefault((y // 16) * gx + x // 16, set()).add(int(index[y, x]))
    out = dict(index=index, depth=depth, z=z, candidate=cand, adjacent=adj, last=last, longest=np.int64(longest),
               margin=f64(m), closest=f64(closest), max_distinct=np.int64(max(len(s) for s in per_tile.values())),
               flip_candidates=np.int64(CC.flip_candidates(name)))
    g = _upstream_on(name, cand)
    dz, means3D = gradient(name, index, g, f64)
    dz32, m32 = restated(name, index, g)
    out.update(dz=dz, means3D=means3D, err_dz=f64(np.linalg.norm(dz32.astype(f64) - dz)),
               err_means3D=f64(np.linalg.norm(m32.astype(f64) - means3D)))
    return out


def _upstream_on(name, candidate):
    _, W, H, seed = AC.SCENES[name][:4]
    g = np.random.default_rng(G_SEED + seed).standard_normal((1, H, W)).astype(f32)
    g[0][candidate] = 0.0
    return g


@functools.lru_cache(maxsize=None)
def upstream(name):
    """g = dL/dmedian_depth: a seeded standard-normal (1,H,W) float32, zero on the fixture's candidate pixels."""
    return _upstream_on(name, fixture_truth(name)["candidate"])


def gradient(name, index, g, dtype):
    """(dz (P,), means3D (P,3)) of sum_pix g median_depth in dtype, the pixels summed in row-major order."""
    n = AC.SCENES[name][0]
    dz = np.zeros(n, dtype)
    on = index >= 0
    np.add.at(dz, index[on], g[0][on].astype(dtype))
    return dz, dz[:, None] * scene(name)["viewmatrix"].astype(dtype)[:3, 2][None, :]


def restated(name, index, g):
    """The same in numpy float32 with the pixels summed in another order (column-major, bottom to top)."""
    n = AC.SCENES[name][0]
    dz = np.zeros(n, f32)
    idx, gg = index.T[:, ::-1].ravel(), g[0].T[:, ::-1].ravel()
    for i, v in zip(idx, gg):
        if i >= 0:
            dz[i] = f32(dz[i] + v)
    return dz, dz[:, None] * scene(name)["viewmatrix"].astype(f32)[:3, 2][None, :]


@functools.lru_cache(maxsize=None)
def fixture_truth(name):
    z = load_golden("median")
    pre = f"{name}_"
    return {k[len(pre):]: v for k, v in z.items() if k.startswith(pre)}


def bar(t, key, suite_bar, norm):
    """The bar of one gradient comparison, as tests/distortion_cases.py's: the larger of the suite's clean bar and
    RESTATEMENT_MARGIN x the float32 restatement's absolute error over `norm`, the L2 norm of the truth compared
    against."""
    return max(suite_bar, RESTATEMENT_MARGIN * float(t[f"err_{key}"]) / norm)


def camera_column(name, dz):
    """dL/dviewmatrix[:, 2] (4,) float64 = sum_i dz_i [p_i, 1]."""
    p = scene(name)["means3D"].astype(f64)
    return np.concatenate([(p * dz[:, None]).sum(0), [dz.sum()]])


# ---- the normal consistency on the blended surface d = (1 - r) D / A + r M ----

def surface_consistency(D, A, N, M, ratio, tanfovx, tanfovy):
    """E (1,H,W) = 1 - stopgrad(A) (N . n_d), n_d the normals of tests/normal_cases.py taken from the blended surface:
    its depth_normals reads d as D / A, so it is handed D' = d A (d = 0 where A == 0), whose quotient is d again."""
    live = A > 0
    d = torch.where(live, (1 - ratio) * (D / torch.where(live, A, torch.ones_like(A))) + ratio * M,
                    torch.zeros_like(D))
    return _consistency_of_surface(d, A, N, tanfovx, tanfovy)


def _consistency_of_surface(d, A, N, tanfovx, tanfovy):
    _, H, W = d.shape
    n = torch.zeros(3, H, W, dtype=d.dtype)
    if H >= 3 and W >= 3:
        rx, ry = NC.rays(H, W, tanfovx, tanfovy, d.dtype)
        Pt = torch.stack([d[0] * rx[None, :], d[0] * ry[:, None], d[0]])
        dv = Pt[:, 2:, 1:-1] - Pt[:, :-2, 1:-1]
        dh = Pt[:, 1:-1, 2:] - Pt[:, 1:-1, :-2]
        c = torch.linalg.cross(dv, dh, dim=0)
        sq = (c * c).sum(0, keepdim=True)
        ok = sq > 0
        unit = torch.where(ok, c * torch.rsqrt(torch.where(ok, sq, torch.ones_like(sq))), torch.zeros_like(c))
        n = torch.nn.functional.pad(unit, (1, 1, 1, 1))
    else:
        n = n + 0 * d
    return 1 - A.detach() * (N * n).sum(0, keepdim=True)


SURFACE_QUANTITIES = ("E", "dD", "dM", "dA", "dN")


def run_surface(D, A, N, M, dE, ratio, tanfovx, tanfovy):
    """(E, dD, dM, dA, dN) of the restatement in the dtype of its arguments."""
    D, A, N, M = (t.detach().clone().requires_grad_(True) for t in (D, A, N, M))
    E = surface_consistency(D, A, N, M, ratio, tanfovx, tanfovy)
    E.backward(dE)
    return E.detach(), D.grad, M.grad, A.grad, N.grad


def surface_bars(inputs, ratio, tanfovx, tanfovy):
    """(float64 reference, bars) of run_surface on float32 `inputs` (D, A, N, M, dE): per quantity NC.BAR_FACTOR x the
    float32 torch route's relative L2 error against float64, at least NC.BAR_FLOOR (tests/test_normals.py's bars)."""
    ref = run_surface(*(t.double() for t in inputs), ratio, tanfovx, tanfovy)
    got = run_surface(*inputs, ratio, tanfovx, tanfovy)
    return ref, tuple(NC.bar_of(a, r) for a, r in zip(got, ref))


# H x W: one backward tile (64 x 16) with room to spare, and a partial tile both ways whose halo crosses the image edge
SURFACE_CASES = (NC.Case("5x7", 5, 7), NC.Case("17x9", 17, 9, seed=3))


@functools.lru_cache(maxsize=None)
def make_surface(case):
    """(D, A, N, M, dE) in float32: tests/normal_cases.py's make() and a median depth within 10 % of the expected depth
    (a surface of its own, as under a floater).  Shared by the tests: do not modify."""
    D, A, N, dE = NC.make(case)
    g = torch.Generator().manual_seed(1000 + case.seed)
    live = A > 0
    z = torch.where(live, D / torch.where(live, A, torch.ones_like(A)), torch.zeros_like(D))
    M = z * (0.9 + 0.2 * torch.rand(1, case.H, case.W, generator=g))
    return D, A, N, M, dE
