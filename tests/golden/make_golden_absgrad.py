#!/usr/bin/env python
"""Ground truth of the absolute screen-space gradients (AbsGS): tests/golden/absgrad.npz.

From this repository's CPU oracle alone (tests/absgrad_cases.py: one backward per pixel with the upstream gradients
masked to it, absolute values summed in float64).  Per scene the fixture holds the truth `<scene>_abs` (P,2) float64,
the signed sum of the same per-pixel calls against the oracle's full backward (`<scene>_signed_residual`, relative
L2: the decomposition's own error), the oracle census the tests assert (`<scene>_census`, JSON), a SHA-256 of the
regenerated inputs and the inputs that are stored rather than regenerated.  Scene A also has its truth without the
inverse-depth gradient (`A_noinv_abs`) and with an alpha gradient and a background image (`A_ext_abs`).

Usage:  python -B tests/golden/make_golden_absgrad.py     (about a minute; scene B is most of it)
"""
from __future__ import annotations

import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

from tests import absgrad_cases as C  # noqa: E402
from tests.helpers import rel_l2  # noqa: E402


def main():
    out = {}
    for name in C.SCENES:
        t0 = time.time()
        inp, _, _ = C.scene(name)
        a, s, full, run = C.truth(name)
        cen = C.census(run)
        cen["abs_over_signed_norm"] = float(np.linalg.norm(a) / np.linalg.norm(full))
        out[f"{name}_abs"] = a
        out[f"{name}_signed_residual"] = np.float64(rel_l2(s, full))
        out[f"{name}_census"] = np.str_(json.dumps(cen, sort_keys=True))
        out[f"{name}_input_sha256"] = np.str_(C.input_hash(name))
        for k in C.STORED_INPUTS:
            out[f"{name}_input_{k}"] = np.asarray(inp[k], np.float32)
        print(f"{name}: {time.time() - t0:.1f} s, signed residual {float(out[name + '_signed_residual']):.2e}, {cen}")
    t0 = time.time()
    out["A_noinv_abs"] = C.truth("A", with_invdepth=False)[0]
    out["A_ext_abs"] = C.truth_ext()[0]
    print(f"A without inverse depth, A with alpha gradient and background image: {time.time() - t0:.1f} s")
    path = os.path.join(REPO, "tests", "golden", "absgrad.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
