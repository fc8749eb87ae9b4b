"""Inputs, references and bars of the fused-SSIM parity tests (tests/test_ssim.py).

Truth is the float64 oracle/ssim_oracle.py on the fp32 inputs.  A bar is never fitted to HIP output: it comes from the
error the three float32 restatements of oracle/ssim_restatements.py (same formulas, three association orders) make on
the same input.  With E the largest of their three errors in a measure:

    mean                       max(4 E, 2e-6)          2e-6 is the bar the suite has always held on noise images
    gradient, max |err|        max(4 E, 8 * 2^-24 T)
    gradient, L2 norm of err   max(4 E, 8 * 2^-24 T)   (the norm over all pixels of all planes)

4 = twice the 2.0x by which a correct fp32 implementation in another FMA order was seen to exceed these restatements
(CPU emulation; at >= 1000 counted pixels per plane and a non-zero gradient).  T (ssim_oracle.ssim(...,
with_term_magnitude=True)) is the largest per-pixel sum of the magnitudes of the three gradient terms: where the true
gradient is 0 (x == y) every implementation returns rounding noise of the order 2^-24 T, and one draw of that noise is
no bound on another.

Seam cases with fewer than 1000 counted pixels per plane do not use their own E (a handful of pixels makes it one draw
of rounding noise): they borrow the gradient bars of the 45x77 noise case in the same padding, times
max(1, 1000 / counted per plane) because g = 1 / counted scales every gradient, and are compared per pixel (and in the
L2 norm against the borrowed L2 bar, scaled the same way).

test_restatements_pass_each_others_bars (no GPU) holds every value case to the leave-one-out version of these bars.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

from oracle import ssim_oracle as SO
from oracle import ssim_restatements as SR

MEAN_FLOOR = 2e-6
FACTOR = 4.0
TERM_FLOOR = 8 * 2.0 ** -24
MIN_COUNTED = 1000
MEASURES = ("mean", "grad_max", "grad_l2")


@dataclass(frozen=True)
class Case:
    name: str
    kind: str      # "value" or "seam"
    gen: str
    shape: tuple   # (B, C, H, W)
    padding: str

    @property
    def counted_per_plane(self) -> int:
        H, W = self.shape[2:]
        return (H - 10) * (W - 10) if self.padding == "valid" else H * W


def noise_images(B, C, H, W, seed):
    """The generator tests/test_ssim.py has always used: uniform noise and the same noise perturbed by N(0, 0.15)."""
    rng = np.random.default_rng(seed)
    gt = rng.random((B, C, H, W))
    render = np.clip(gt + 0.15 * rng.standard_normal((B, C, H, W)), 0, 1)
    return render.astype(np.float32), gt.astype(np.float32)


def _edge(shape, at):
    e = np.full(shape, 0.2, np.float32)
    e[..., at:] = 0.8
    return e


def _generate(gen: str, shape: tuple):
    B, C, H, W = shape
    x, y = noise_images(B, C, H, W, seed=7)
    f32 = np.float32
    if gen == "noise":
        return x, y
    if gen == "flat":
        return np.full(shape, 0.3, f32), np.full(shape, 0.7, f32)
    if gen == "flat_noisy":
        rng = np.random.default_rng(8)
        return (0.9 + 1e-3 * rng.standard_normal(shape)).astype(f32), np.full(shape, 0.9, f32)
    if gen == "edge":
        return _edge(shape, W // 2 + 1), _edge(shape, W // 2)
    if gen == "black_vs_noise":
        return np.zeros(shape, f32), y
    if gen == "hdr":
        return x * f32(8), y * f32(8)
    if gen == "negative":
        return x - f32(0.5), y - f32(0.5)
    if gen == "same_noise":
        return y.copy(), y
    if gen == "same_flat":
        return np.ones(shape, f32), np.ones(shape, f32)
    if gen == "black":
        return np.zeros(shape, f32), np.zeros(shape, f32)
    raise KeyError(gen)


VALUE_GENS = ("noise", "flat", "flat_noisy", "edge", "black_vs_noise", "hdr", "negative", "same_noise", "same_flat",
              "black")
VALUE_SHAPES = ((45, 77), (64, 128))
SEAM_H = (1, 5, 10, 11, 15, 16, 17, 31, 32, 33, 36, 37, 43)
SEAM_W = (1, 5, 10, 11, 31, 32, 33, 59, 63, 64, 65, 69, 70, 74, 75, 128, 129)


def _seam_shapes():
    s = [(h, w) for h in SEAM_H for w in (11, 65, 129)] + [(h, w) for h in (11, 33) for w in SEAM_W]
    s += [(1, 1), (1, 129), (43, 1)]
    return sorted(set(s))


def _cases():
    out = []
    for gen in VALUE_GENS:
        for H, W in VALUE_SHAPES:
            for padding in ("same", "valid"):
                out.append(Case(f"{gen}-{H}x{W}-{padding}", "value", gen, (1, 2, H, W), padding))
    for H, W in _seam_shapes():
        for padding in ("same", "valid"):
            if padding == "valid" and not (H > 10 and W > 10):
                continue
            out.append(Case(f"seam-{H}x{W}-{padding}", "seam", "noise", (1, 2, H, W), padding))
    for padding in ("same", "valid"):
        out.append(Case(f"seam-planes2x3-33x65-{padding}", "seam", "noise", (2, 3, 33, 65), padding))
    return tuple(out)


CASES = _cases()
VALUE_CASES = tuple(c for c in CASES if c.kind == "value")
BY_NAME = {c.name: c for c in CASES}


def errors(mean, grad, ref_mean, ref_grad) -> dict:
    """The three measures of (mean, grad) against the float64 reference."""
    d = np.asarray(grad, np.float64) - ref_grad
    return {"mean": abs(float(mean) - ref_mean), "grad_max": float(np.abs(d).max()),
            "grad_l2": float(np.sqrt(np.sum(d * d)))}


@functools.lru_cache(maxsize=None)
def inputs(case: Case):
    x, y = _generate(case.gen, case.shape)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


@functools.lru_cache(maxsize=None)
def reference(case: Case):
    """(mean, dmean/dimg1, T) of the float64 oracle; computed once and shared."""
    x, y = inputs(case)
    mean, grad, T = SO.ssim(x, y, case.padding, with_term_magnitude=True)
    grad.setflags(write=False)
    return mean, grad, T


@functools.lru_cache(maxsize=None)
def restatement_errors(case: Case) -> dict:
    """{order: {measure: error}} of the three float32 restatements against the oracle."""
    x, y = inputs(case)
    ref_mean, ref_grad, _ = reference(case)
    return {o: errors(*SR.ssim(x, y, case.padding, order=o), ref_mean, ref_grad) for o in SR.ORDERS}


def bars_from(case: Case, orders) -> dict:
    """The bars of `case` built from the restatements named in `orders`."""
    err = restatement_errors(case)
    E = {m: max(err[o][m] for o in orders) for m in MEASURES}
    floor = TERM_FLOOR * reference(case)[2]
    return {"mean": max(FACTOR * E["mean"], MEAN_FLOOR), "grad_max": max(FACTOR * E["grad_max"], floor),
            "grad_l2": max(FACTOR * E["grad_l2"], floor)}


@functools.lru_cache(maxsize=None)
def _bar(case: Case):
    out = bars_from(case, SR.ORDERS)
    if case.counted_per_plane < MIN_COUNTED:
        donor = bars_from(BY_NAME[f"noise-45x77-{case.padding}"], SR.ORDERS)
        scale = max(1.0, MIN_COUNTED / case.counted_per_plane)
        out["grad_max"], out["grad_l2"] = scale * donor["grad_max"], scale * donor["grad_l2"]
    return out


def bar(case: Case, upstream: float = 1.0) -> dict:
    """{measure: allowance} of a case; the gradient allowances scale with |upstream| (dL/dmean), the mean's does not."""
    b = dict(_bar(case))
    b["grad_max"] *= abs(upstream)
    b["grad_l2"] *= abs(upstream)
    return b
