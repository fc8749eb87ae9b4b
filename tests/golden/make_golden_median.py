#!/usr/bin/env python
"""Ground truth of the median depth map and its gradient: tests/golden/median.npz.

From this repository's CPU oracle alone (tests/median_cases.py: each pixel's contributors front to back with the
oracle's own weights, the incoming transmittance 1 - sum_(j<i) w_j in float64, the median the last contributor with
that above 0.5, its depth the oracle's).  Per scene of tests/absgrad_cases.py the fixture holds, under `<scene>_`:
`index` (H,W) int32 and `depth` (H,W) float32 (-1 and 0 where no Gaussian reaches), `z` (P,) float32 the oracle's view depths, `candidate` (H,W) bool (an
incoming transmittance within `margin` of 0.5) with `adjacent` (H,W,2) the two ids such a pixel may select,
`last` (H,W) bool (the median is the pixel's last contributor), `longest`, `margin`, `closest`, `max_distinct`, `flip_candidates` (0), and under the seeded
upstream gradient of median_cases.upstream (zero on the candidates) `dz` (P,) and `means3D` (P,3) in float64 with the
float32 restatement's absolute errors `err_dz`, `err_means3D`, from which the tests derive their bars.  Also a
SHA-256 of each scene's upstream gradient.

Usage:  python -B tests/golden/make_golden_median.py     (a few minutes; scene B is most of it)
"""
from __future__ import annotations

import hashlib
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

from tests import median_cases as MC  # noqa: E402


def main():
    out = {}
    for name in MC.SCENES:
        t0 = time.time()
        t = MC.truth(name)
        for k, v in t.items():
            out[f"{name}_{k}"] = v
        g = MC._upstream_on(name, t["candidate"])
        out[f"{name}_g_sha256"] = np.str_(hashlib.sha256(g.tobytes()).hexdigest())
        print(f"{name}: {time.time() - t0:.1f} s, pixels {t['index'].size}, untouched {int((t['index'] < 0).sum())}, "
              f"median is the last contributor {int(t['last'].sum())}, longest list {int(t['longest'])}, margin "
              f"{float(t['margin']):.3g}, closest to 0.5 {float(t['closest']):.3g}, candidates "
              f"{int(t['candidate'].sum())}, most distinct medians in a tile {int(t['max_distinct'])}, Gaussians with a "
              f"gradient {int(np.count_nonzero(t['dz']))}, restatement error means3D "
              f"{float(t['err_means3D']) / float(np.linalg.norm(t['means3D'])):.3g}")
    path = os.path.join(REPO, "tests", "golden", "median.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
