"""conic_is_definite (csrc/gsr_common.h) against the compositing exponent it vouches for, on the CPU.

The composites run a walk body without the `power2 <= 0` test for batches whose staged instances all pass
conic_is_definite (knob definite_fast).  That is only the same computation if no conic the classifier passes can give a
positive (or NaN) exponent at any pixel.  Here the classifier, the staging (stage_rec_a / stage_rec_b) and power2_at are
restated in numpy fp32 in the kernels' operation order (fmaf as a float64 product plus add, rounded once to fp32), as
tools/cell_stats.py restates strip_mask_exact, and swept over conics with eigenvalue ratios from 1 down to 1e-9 -- far
past the 12 * 2^-24 = 7.2e-7 below which rounding can make the exponent positive -- with pixel offsets at the places
where it does: along the ellipse's long axis (on lattice directions, so that integer pixels lie on it), up to 2^15 px
away, exactly zero, and a fraction of a pixel from the centre."""
import os
import re

import numpy as np

f32 = np.float32
NEG_HALF_LOG2E = f32(-0.72134752044448170)
NEG_LOG2E = f32(-1.4426950408889634)
COMMON_H = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gaussian_splatting_lightning_amd",
                        "csrc", "gsr_common.h")
TAU = f32(1e-4)
RATIOS = [10.0 ** -k for k in range(10)]
PER_RATIO = 8000  # conics per ratio and offset family: 10 x 4 x 8000 = 320 k exponents


def conic_is_definite(x, y, a, b, c, o, col0, row0):
    """gsr_common.h conic_is_definite in numpy fp32 (uncontracted there, so the same bits)."""
    x, y, a, b, c, o, col0, row0 = (np.asarray(v, f32) for v in (x, y, a, b, c, o, col0, row0))
    with np.errstate(all="ignore"):
        det = a * c - b * b
        hd, hs = f32(0.5) * (a - c), f32(0.5) * (a + c)
        rad = np.sqrt(hd * hd + b * b)
        lmin, lmax = hs - rad, hs + rad
        return ((a > 0) & (c > 0) & (det > 0) & (lmax <= f32(1024)) & (lmin >= TAU * lmax) & (lmin >= f32(2.0 ** -30)) &
                (np.abs(x - col0) <= f32(32768)) & (np.abs(y - row0) <= f32(32768)) & (np.abs(x) >= f32(2.0 ** -16)) &
                (np.abs(y) >= f32(2.0 ** -16)) & (np.abs(o) <= f32(3.0e38)))


def fmaf(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def power2_at_pixel(x, y, a, b, c, px, py):
    """The composites' exponent at pixel (px, py): stage_rec_a / stage_rec_b, then P0, L and power2_at."""
    x, y, a, b, c, px, py = (np.asarray(v, f32) for v in (x, y, a, b, c, px, py))
    with np.errstate(all="ignore"):
        A, B, C = a * NEG_HALF_LOG2E, b * NEG_LOG2E, c * NEG_HALF_LOG2E
        dx = x - px
        P0, L = (A * dx) * dx, B * dx
        dy = y - py
        return fmaf(dy, fmaf(C, dy, L), P0)


def _conics(rng, ratio, n):
    """n conics (fp32 a, b, c) with eigenvalues lmax, ratio * lmax, and the unit vector of their long axis (the
    eigenvector of the small eigenvalue).  Half of the axes lie on lattice directions (q, p), so that the integer pixels
    (q k, p k) from an integer centre are on the axis."""
    lmax = np.exp(rng.uniform(np.log(1e-4), np.log(1 / 0.3), n))
    lmax[: n // 8] = 1 / 0.3  # the largest the reference's +0.3 dilation admits
    lmin = lmax * ratio
    p, q = rng.integers(-7, 8, n), rng.integers(1, 8, n)
    th = np.where(rng.random(n) < 0.5, np.arctan2(p, q), rng.uniform(0, np.pi, n))
    ux, uy = np.cos(th), np.sin(th)  # long axis
    a = lmin * ux * ux + lmax * uy * uy
    b = (lmin - lmax) * ux * uy
    c = lmin * uy * uy + lmax * ux * ux
    return a.astype(f32), b.astype(f32), c.astype(f32), ux, uy, p, q, th


def _samples():
    """(x, y, a, b, c, px, py) over every ratio and offset family."""
    rng = np.random.default_rng(1234)
    out = []
    for ratio in RATIOS:
        n = PER_RATIO
        # along the long axis, on the lattice where the axis is a lattice direction, up to ~3000 px
        a, b, c, ux, uy, p, q, th = _conics(rng, ratio, n)
        px, py = rng.integers(0, 4096, n), rng.integers(0, 4096, n)
        k = rng.integers(1, 400, n)
        lattice = np.isclose(th, np.arctan2(p, q))
        t = rng.uniform(1, 3000, n)
        x = np.where(lattice, px + q * k, np.rint(px + ux * t)).astype(f32)
        y = np.where(lattice, py + p * k, np.rint(py + uy * t)).astype(f32)
        out.append((x, y, a, b, c, px, py))
        # anywhere up to 2^15 px away (and beyond the classifier's range), fractional centres
        a, b, c, *_ = _conics(rng, ratio, n)
        px, py = rng.integers(0, 32768, n), rng.integers(0, 32768, n)
        x = (px + rng.uniform(-40000, 40000, n)).astype(f32)
        y = (py + rng.uniform(-40000, 40000, n)).astype(f32)
        out.append((x, y, a, b, c, px, py))
        # exactly on the pixel centre
        a, b, c, *_ = _conics(rng, ratio, n)
        px, py = rng.integers(1, 32768, n), rng.integers(1, 32768, n)
        out.append((px.astype(f32), py.astype(f32), a, b, c, px, py))
        # a fraction of a pixel away, down to the last bits of the coordinate, along the long axis
        a, b, c, ux, uy, *_ = _conics(rng, ratio, n)
        px, py = rng.integers(1, 4096, n), rng.integers(1, 4096, n)
        t = np.exp(rng.uniform(np.log(1e-4), np.log(2.0), n))
        out.append(((px + ux * t).astype(f32), (py + uy * t).astype(f32), a, b, c, px, py))
    return tuple(np.concatenate([s[i] for s in out]) for i in range(7))


def test_restated_constants_are_the_headers():
    src = open(COMMON_H).read()
    assert f32(float(re.search(r"DEFINITE_TAU = ([0-9.e+-]+)f;", src).group(1))) == TAU
    assert f32(float(re.search(r"NEG_HALF_LOG2E = (-[0-9.]+)f;", src).group(1))) == NEG_HALF_LOG2E
    assert f32(float(re.search(r"NEG_LOG2E = (-[0-9.]+)f;", src).group(1))) == NEG_LOG2E
    body = src[src.index("bool conic_is_definite("):]
    body = body[:body.index("\n}\n")]
    for lit in ("1024.f", "0x1p-30f", "32768.f", "0x1p-16f", "3.0e38f", "fp contract(off)"):
        assert lit in body, lit


def test_no_definite_conic_gives_a_positive_exponent():
    x, y, a, b, c, px, py = _samples()
    assert len(x) <= 400_000
    col0, row0 = (px // 16 * 16).astype(f32), (py // 16 * 16).astype(f32)
    definite = conic_is_definite(x, y, a, b, c, np.full(len(x), 0.5, f32), col0, row0)
    p2 = power2_at_pixel(x, y, a, b, c, px, py)
    positive = p2 > 0
    # the sweep reaches both sides: exponents that rounding made positive, and conics the classifier passes, at
    # every ratio well above TAU
    ratio = np.repeat(RATIOS, 4 * PER_RATIO)
    assert positive.sum() > 100 and definite.sum() > 50_000, (positive.sum(), definite.sum())
    for r in (1.0, 1e-1, 1e-2, 1e-3):
        assert definite[ratio == r].mean() > 0.5, (r, definite[ratio == r].mean())
    assert not positive[ratio >= 0.5e-6].any(), "a positive exponent above the derived bound of 7.2e-7"
    # the two statements of the issue: none of the definite ones is positive (or NaN), every positive one is rejected
    assert not (definite & ~(p2 <= 0)).any()
    assert not definite[positive].any()
    # and the margin: nothing the classifier passes is within 16 x of the ratio where the positives begin
    assert not definite[ratio < 16 * 7.2e-7].any()


def test_exponent_is_zero_on_the_centre_and_never_nan_in_range():
    rng = np.random.default_rng(5)
    a, b, c, *_ = _conics(rng, 0.3, 4000)
    px, py = rng.integers(1, 32768, 4000), rng.integers(1, 32768, 4000)
    p2 = power2_at_pixel(px.astype(f32), py.astype(f32), a, b, c, px, py)
    assert (p2 == 0).all()
    # the largest terms the classifier admits: lmax = 2^10 at 2^15 + 15 px stay finite (no inf - inf)
    big = f32(1024.0)
    p2 = power2_at_pixel(f32(1.0), f32(1.0), big, f32(0), big, f32(32768 + 16), f32(32768 + 16))
    assert np.isfinite(p2) and p2 < 0


def test_everything_unprovable_is_rejected():
    one, z = f32(1.0), f32(0.0)
    ok = dict(x=f32(100.5), y=f32(50.25), a=one, b=f32(0.2), c=f32(0.7), o=f32(0.5), col0=f32(96), row0=f32(48))
    assert conic_is_definite(**ok)
    nan, inf = f32(np.nan), f32(np.inf)
    bad = [dict(a=nan), dict(b=nan), dict(c=nan), dict(a=inf), dict(c=inf), dict(b=inf), dict(o=nan), dict(o=inf),
           dict(o=-inf), dict(x=nan), dict(y=nan), dict(x=inf), dict(a=-one), dict(c=-one), dict(a=z), dict(c=z),
           dict(b=one),  # det = 0.7 - 1 < 0
           dict(b=f32(np.sqrt(0.7))),  # det ~ 0
           dict(a=f32(2048), c=f32(2048)),  # lmax > 2^10
           dict(a=f32(1e-10), b=z, c=f32(1e-10)),  # lmin < 2^-30
           dict(a=one, b=z, c=f32(0.99e-4)),  # ratio < TAU
           dict(x=f32(96 + 32769)), dict(y=f32(48 - 32769)),  # centre out of range of the tile
           dict(x=f32(1e-6), col0=z), dict(y=f32(-1e-6), row0=z), dict(x=z, col0=z)]  # offsets that can go subnormal
    for d in bad:
        assert not conic_is_definite(**{**ok, **d}), d
    assert conic_is_definite(**{**ok, **dict(a=one, b=z, c=f32(1.01e-4))})
    assert conic_is_definite(**{**ok, **dict(o=f32(-0.5))})  # a finite opacity of any sign: alpha < 1/255 either way
