#!/usr/bin/env python
"""Ground truth of the per-Gaussian contribution statistics: tests/golden/contrib.npz.

From this repository's CPU oracle alone (tests/contrib_cases.py: one backward per three pixels, each with a single 1 in
one colour channel, so the colour gradient IS the compositing weight of every Gaussian at those pixels; counts, sums and
maxima formed in float64).  Per scene of tests/absgrad_cases.py the fixture holds `<scene>_count` (P,) int64,
`<scene>_wsum` and `<scene>_wmax` (P,) float64, the same three under the scene's weight image as `<scene>_m_*`, the
number of threshold-flip candidates (`<scene>_flip_candidates`, 0) and a SHA-256 of the weight image.

Usage:  python -B tests/golden/make_golden_contrib.py     (about a minute; scene B is most of it)
"""
from __future__ import annotations

import hashlib
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

from tests import contrib_cases as C  # noqa: E402


def main():
    out = {}
    for name in C.SCENES:
        t0 = time.time()
        t = C.truth(name)
        for k, v in t.items():
            out[f"{name}_{k}"] = v
        out[f"{name}_flip_candidates"] = np.int64(C.flip_candidates(name))
        out[f"{name}_weights_sha256"] = np.str_(hashlib.sha256(C.weights(name).tobytes()).hexdigest())
        m = C.weights(name)
        print(f"{name}: {time.time() - t0:.1f} s, flips {int(out[name + '_flip_candidates'])}, "
              f"taken {int((t['count'] > 0).sum())} of {len(t['count'])} Gaussians, pairs {int(t['count'].sum())}, "
              f"weights: {float((m == 0).mean()):.2f} zero, {float((m < 0).mean()):.3f} negative, "
              f"max wmax {float(t['wmax'].max()):.4f}")
    path = os.path.join(REPO, "tests", "golden", "contrib.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
