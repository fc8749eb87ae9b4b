#!/usr/bin/env python
"""Camera-gradient golden vectors from the REFERENCE Python rasterizer: tests/golden/camgrad.npz.

Runs only in the build container, where the reference exists; it imports `gs_lightning.rasterize` with the shims of
make_golden.py (no reference code is copied) and stores OUTPUTS only: the reference's autograd gradients with respect
to `viewmatrix`, `projmatrix` and `campos` as three independent leaves, for the cases of tests/camera_cases.py:

  * unsat_sh3_150x100 and unsat_deg1of3_96x80, on the inputs and upstream gradients those fixtures hold (SH padded to
    25 coefficients as make_golden.reference_fwd_bwd does; scale_modifier 0.8 in the second);
  * big_sh3_208x144: a scene in which some Gaussians cover more than 64 tiles (their gradient sums take the separate
    big-Gaussian path).  The upstream gradients are zeroed on the oracle's threshold-flip candidate pixels
    (threshold_margin() < FLIP_EXCLUDE, as make_golden_ref.py does); the mask is stored as bits, with a SHA-256 of the
    regenerated inputs.  No pixel of it may terminate (the reference's and the CUDA semantics' rules then coincide):
    asserted here from the oracle's final transmittance.

Usage:  python -B tests/golden/make_golden_camera.py 2>/dev/null
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
sys.dont_write_bytecode = True

from make_golden import _import_reference  # noqa: E402

from tests.camera_cases import (BIG_CASE, BIG_GAUSSIAN_TILES, CAMERA_KEYS, UNSAT_CASES, big_case_inputs,  # noqa: E402
                                input_sha256)
from tests.helpers import FLIP_EXCLUDE, T_KEEP, golden_inputs, load_golden, run_oracle  # noqa: E402


def reference_camera_grads(R, inp, dc, di, dtype=torch.float32):
    """The reference's d loss / d (viewmatrix, projmatrix, campos), loss = sum(image dc) + sum(invdepth di); also its
    dL/dmeans3D (the translation identity's check)."""
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype)  # noqa: E731
    cam = {k: t(inp[k]).requires_grad_(True) for k in CAMERA_KEYS}
    means = t(inp["means3D"]).requires_grad_(True)
    shs = t(inp["shs"])
    N, M = shs.shape[:2]
    shs = torch.cat([shs, torch.zeros(N, 25 - M, 3, dtype=dtype)], 1) if M < 25 else shs
    img, _radius, depth = R.rasterize_gaussian(
        means3D=means, opacities=t(inp["opacities"]), scales=t(inp["scales"]), rotations=t(inp["rotations"]),
        shs=shs, scale_modifier=inp["scale_modifier"], image_width=inp["image_width"],
        image_height=inp["image_height"], tanfovx=inp["tanfovx"], tanfovy=inp["tanfovy"], background=t(inp["bg"]),
        sh_degree=inp["sh_degree"], **cam)
    ((img * t(dc)).sum() + (depth * t(di)).sum()).backward()
    out = {k: v.grad.numpy() for k, v in cam.items()}
    out["means3D"] = means.grad.numpy()
    return out


def main():
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    os.environ.setdefault("TQDM_DISABLE", "1")
    R, _RR = _import_reference()
    rec = {}
    cases = []
    for name in UNSAT_CASES:
        z = load_golden(name)
        cases.append((name, golden_inputs(z), z["dL_dcolor"], z["dL_dinvdepth"]))
    inp, dc, di = big_case_inputs()
    o = run_oracle(inp)
    tiles_max = int(o[3].geom()["tiles_touched"].max())
    assert tiles_max > BIG_GAUSSIAN_TILES, f"no Gaussian above {BIG_GAUSSIAN_TILES} instances after the filter ({tiles_max})"
    t_min = float(o[3].image_state()[0].min())
    assert t_min >= T_KEEP, f"a pixel may terminate (min final T {t_min})"
    mask = o[3].threshold_margin() >= FLIP_EXCLUDE
    rec[BIG_CASE + "_mask_bits"] = np.packbits(mask.reshape(-1))
    rec[BIG_CASE + "_input_sha256"] = np.array(input_sha256(inp, dc, di))
    m = mask.astype(np.float32)
    cases.append((BIG_CASE, inp, dc * m, di * m))
    print(f"{BIG_CASE}: N={len(inp['means3D'])} max tiles {tiles_max}, min final T {t_min:.3f}, "
          f"{int((~mask).sum())} of {mask.size} pixels masked")
    for name, inp, dc, di in cases:
        g32 = reference_camera_grads(R, inp, dc, di)
        g64 = reference_camera_grads(R, inp, dc, di, torch.float64)
        for k in CAMERA_KEYS:
            rec[f"{name}_{k}"] = g32[k].astype(np.float32)
            err = np.linalg.norm(g32[k] - g64[k]) / np.linalg.norm(g64[k])
            print(f"{name} {k}: |g| {np.linalg.norm(g64[k]):.4g}, f32 vs f64 relative L2 {err:.2e}")
        assert not g32["viewmatrix"][:, 3].any() and not g32["projmatrix"][:, 2].any(), "structural zeros"
    path = os.path.join(HERE, "camgrad.npz")
    np.savez_compressed(path, **rec)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
