"""The camera-gradient cases shared by tests/golden/make_golden_camera.py (which writes tests/golden/camgrad.npz from
the reference rasterizer) and the tests that read it: inputs, upstream gradients and the fixture's loader."""
from __future__ import annotations

import hashlib

import numpy as np
import torch

from tests.helpers import golden_inputs, load_golden, scene_inputs, upstream

CAMERA_KEYS = ("viewmatrix", "projmatrix", "campos")
UNSAT_CASES = ("unsat_sh3_150x100", "unsat_deg1of3_96x80")  # inputs and upstream gradients: those fixtures' own
BIG_CASE = "big_sh3_208x144"  # some Gaussians above BIG_GAUSSIAN_TILES (64) tile instances: their sums come from bigsum
CASES = UNSAT_CASES + (BIG_CASE,)
BIG_GAUSSIAN_TILES = 64
PER_GAUSSIAN = ("means3D", "opacities", "scales", "rotations", "shs")


def big_case_inputs():
    """(inputs, dL_dcolor, dL_dinvdepth) of BIG_CASE before the fixture's pixel mask: a low-opacity scene with a tenth
    of stress Gaussians (large ones among them), the Gaussians with z_view <= 0.5 dropped."""
    W, H, seed = 208, 144, 7
    inp = scene_inputs(300, W, H, sh_degree=3, seed=seed, opacity_scale=0.02, bg=(0.2, 0.5, 0.9), stress_fraction=0.1)
    means = torch.from_numpy(inp["means3D"])
    ph = torch.cat([means, torch.ones(len(means), 1)], 1) @ torch.from_numpy(inp["viewmatrix"])
    keep = (ph[:, 2] > 0.5).numpy()
    for k in PER_GAUSSIAN:
        inp[k] = np.ascontiguousarray(inp[k][keep])
    dc, di = upstream(W, H, seed)
    return inp, dc, di


def input_sha256(inp, dc, di) -> str:
    h = hashlib.sha256()
    for a in (inp["means3D"], inp["shs"], dc, di):
        h.update(np.ascontiguousarray(a, np.float32).tobytes())
    return h.hexdigest()


def load_case(name: str, fixture: dict):
    """(inputs, dL_dcolor, dL_dinvdepth, {viewmatrix, projmatrix, campos: the reference's gradient}) of one case."""
    if name == BIG_CASE:
        inp, dc, di = big_case_inputs()
        h = input_sha256(inp, dc, di)
        assert h == str(fixture[name + "_input_sha256"]), f"{name}: regenerated inputs differ from the generator's ({h})"
        W, H = inp["image_width"], inp["image_height"]
        mask = np.unpackbits(fixture[name + "_mask_bits"])[:W * H].reshape(H, W).astype(np.float32)
        dc, di = dc * mask, di * mask
    else:
        z = load_golden(name)
        inp, dc, di = golden_inputs(z), z["dL_dcolor"], z["dL_dinvdepth"]
    return inp, dc, di, {k: fixture[f"{name}_{k}"] for k in CAMERA_KEYS}


def translation_residual(V, P, g_means3D_sum, g_view, g_proj, g_campos, g_means3D_abs_sum):
    """The translation identity's residual and its scale, per component.  Moving every mean and the camera position
    by d while row 3 of the view and projection matrices takes -d V[:3,:] and -d P[:3,:] changes nothing, so
        sum_g dL/dmeans3D_g + dL/dcampos - V[:3,:] dV[3,:] - P[:3,:] dP[3,:] = 0
    exactly in real arithmetic.  Scale: sum_g |dL/dmeans3D_g| + |dL/dcampos|."""
    f8 = lambda a: np.asarray(a, np.float64)  # noqa: E731
    res = f8(g_means3D_sum) + f8(g_campos) - f8(V)[:3, :] @ f8(g_view)[3, :] - f8(P)[:3, :] @ f8(g_proj)[3, :]
    return res, f8(g_means3D_abs_sum) + np.abs(f8(g_campos))
