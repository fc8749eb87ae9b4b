"""float32 restatements of oracle/ssim_oracle.py -- TEST INFRASTRUCTURE ONLY (the yardstick of tests/ssim_cases.py).

Three numpy float32 evaluations of the same SSIM mean and gradient, written with the formulas an fp32 implementation
uses (moments as E[x^2] - mu^2, one reciprocal of Cc * D, the three per-pixel derivative maps filtered and combined with
x and y) and differing only in the order in which the 11 + 11 filter taps are added:

    "hv_up"     horizontal pass then vertical pass, taps added in increasing order
    "hv_down"   horizontal then vertical, taps added in decreasing order
    "vh_pairs"  vertical then horizontal, taps added pairwise from the outside in: (w0 p0 + w10 p10) + (w1 p1 + w9 p9) ...

Their errors against the float64 oracle say what rounding alone costs on a given input; the spread between them says
how much of that is the order of the sums.  Nothing here is taken from the HIP kernels' output.
"""
from __future__ import annotations

import numpy as np

from oracle import ssim_oracle as SO

F = np.float32
ORDERS = ("hv_up", "hv_down", "vh_pairs")
C1, C2 = F(0.01) * F(0.01), F(0.03) * F(0.03)


def window() -> np.ndarray:
    return SO.window().astype(F)


def _taps(p: np.ndarray, axis: int, n: int, order: str) -> np.ndarray:
    """11-tap filter of the padded array p along `axis` (n outputs), float32 throughout."""
    w = window()
    idx = [slice(None)] * p.ndim

    def term(k):
        idx[axis] = slice(k, k + n)
        return w[k] * p[tuple(idx)]

    if order == "vh_pairs":
        acc = term(0) + term(10)
        for k in range(1, SO.R):
            acc = acc + (term(k) + term(10 - k))
        return acc + term(SO.R)
    ks = range(11) if order == "hv_up" else range(10, -1, -1)
    acc = None
    for k in ks:
        acc = term(k) if acc is None else acc + term(k)
    return acc


def _filt(img: np.ndarray, order: str) -> np.ndarray:
    assert img.dtype == F
    H, W = img.shape[-2:]
    R = SO.R
    p = np.zeros(img.shape[:-2] + (H + 2 * R, W + 2 * R), F)
    p[..., R:R + H, R:R + W] = img
    if order == "vh_pairs":
        return _taps(_taps(p, -2, H, order), -1, W, order)
    return _taps(_taps(p, -1, W, order), -2, H, order)


def ssim(img1, img2, padding="same", upstream=1.0, order="hv_up"):
    """(mean SSIM as a float, upstream * dmean/dimg1 as a float32 array) of (B,C,H,W) float32 arrays."""
    assert order in ORDERS
    x, y = np.asarray(img1, F), np.asarray(img2, F)
    m1, m2 = _filt(x, order), _filt(y, order)
    s11, s22, s12 = _filt(x * x, order) - m1 * m1, _filt(y * y, order) - m2 * m2, _filt(x * y, order) - m1 * m2
    A, B = F(2) * m1 * m2 + C1, F(2) * s12 + C2
    Cc, D = m1 * m1 + m2 * m2 + C1, s11 + s22 + C2
    inv_cd = F(1) / (Cc * D)
    m = A * B * inv_cd
    mask = np.ones(x.shape[-2:], bool)
    if padding == "valid":
        mask[:] = False
        mask[SO.R:-SO.R, SO.R:-SO.R] = True
    n = m.shape[0] * m.shape[1] * int(mask.sum())
    mean = float(np.where(mask, m, F(0)).sum(dtype=F) / F(n))
    g = F(upstream) * F(1.0 / n)
    d12 = F(2) * A * inv_cd
    d11 = -m / D
    dmu = F(2) * m2 * B * inv_cd - F(2) * m1 * m / Cc - F(2) * m1 * d11 - m2 * d12
    zero = F(0)
    grad = (_filt(np.where(mask, g * dmu, zero), order) + F(2) * x * _filt(np.where(mask, g * d11, zero), order)
            + y * _filt(np.where(mask, g * d12, zero), order))
    assert grad.dtype == F
    return mean, grad
