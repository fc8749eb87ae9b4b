#!/usr/bin/env python
"""Ground truth of the depth distortion map and its gradients: tests/golden/distortion.npz.

From this repository's CPU oracle alone (tests/distortion_cases.py: the oracle's own per-pixel weights, D, dD/dw and
dD/dt formed from them in float64, the gradient through the weights from oracle runs with the frozen dD/dw as
precomputed colours, the depth part analytically).  Per scene of tests/absgrad_cases.py and map ("z", "ndc") the
fixture holds, under `<scene>_<map>_`: `D` (H,W), the gradients of sum_pix g D `means3D`, `means2D`, `opacities`,
`scales`, `rotations` and the per-Gaussian depth gradient `dz`, all float64; `flip_candidates` (0); and the errors of
the two float32 restatements ("prefix", "suffix") against that truth as `err_<order>_D` (max over the pixels of
|D - truth| / max(1, |truth|)) and `err_<order>_<tensor>` (L2 norm of the difference), from which the tests derive
their bars.  Also a SHA-256 of each scene's upstream gradient g.

Usage:  python -B tests/golden/make_golden_distortion.py     (a few minutes; scene B is most of it)
"""
from __future__ import annotations

import hashlib
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

from tests import distortion_cases as DC  # noqa: E402


def main():
    out = {}
    for name in DC.SCENES:
        out[f"{name}_g_sha256"] = np.str_(hashlib.sha256(DC.upstream(name).tobytes()).hexdigest())
        for which in DC.MAPS:
            t0 = time.time()
            t = DC.truth(name, which)
            for k, v in t.items():
                out[f"{name}_{which}_{k}"] = v
            rel = {k: DC.restatement_error(t, k) / float(np.linalg.norm(t[k])) for k in DC.GEOMETRY}
            print(f"{name} {which}: {time.time() - t0:.1f} s, flips {int(t['flip_candidates'])}, max D "
                  f"{float(t['D'].max()):.4f}, Gaussians with a gradient "
                  f"{int(np.count_nonzero(np.abs(t['means3D']).sum(1)))} of {t['means3D'].shape[0]}, restatement "
                  f"errors: D {DC.restatement_error(t, 'D'):.3g}, "
                  + ", ".join(f"{k} {v:.3g}" for k, v in rel.items()))
    path = os.path.join(REPO, "tests", "golden", "distortion.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
