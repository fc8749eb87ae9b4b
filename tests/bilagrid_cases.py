"""Reference and case table of the bilateral-grid tests (tests/test_bilagrid_host.py, tests/test_bilagrid.py).

The reference is the definition of include/gsrast.h in torch on the CPU, stated twice: through `F.grid_sample`
(`slice_grid_sample`: mode="bilinear", align_corners=True, padding_mode="border" at ((x, y, gray) - 0.5) * 2) and as
the explicit sum over lattice vertices of hat-function products (`slice_hat`).  `reference()` runs both in float64,
asserts that they agree (outputs and both gradients) and returns the grid_sample one, so the yardstick is checked
against itself without a GPU.  The same `slice_grid_sample` in float32 is the "torch route" whose own error against
float64 sets every bar: the HIP result must be within BAR_FACTOR times it, per quantity.

Input condition.  The case seeds are chosen so that, in float64, every pixel has gray at least MARGIN from 0 and 1 and
every in-range pixel (0 < gray < 1) of a grid with L > 1 has uz at least MARGIN from an integer: no float32 evaluation
lands on the other side of a kink, so no pixel is ever excluded from a comparison.  `make()` asserts the condition.
(With L = 1, uz is 0 everywhere and nothing depends on it.)
"""
from __future__ import annotations

import functools
from typing import NamedTuple, Tuple

import torch
import torch.nn.functional as F

BAR_FACTOR = 4.0  # a different but fixed summation order; the sums have at most a few thousand terms at these shapes
MARGIN = 1e-4
GRAY = (0.299, 0.587, 0.114)


class Case(NamedTuple):
    name: str
    L: int
    Gh: int
    Gw: int
    H: int
    W: int
    idx: Tuple[int, ...] = (0,)
    num: int = 1
    seed: int = 0


# L x Gh x Gw, H x W: what each reaches is in the docstring of tests/test_bilagrid.py
CASES = (
    Case("8x16x16-37x53", 8, 16, 16, 37, 53, seed=0),
    Case("8x16x16-5x7", 8, 16, 16, 5, 7, seed=0),
    Case("1x1x1-4x4", 1, 1, 1, 4, 4, seed=0),
    Case("3x1x5-9x130", 3, 1, 5, 9, 130, seed=0),
    Case("2x2x3-40x300", 2, 2, 3, 40, 300, seed=11),
    Case("8x16x16-64x96-batch", 8, 16, 16, 64, 96, idx=(2, 0, 2), num=4, seed=202),
    # more levels than one grid-gradient workgroup holds (two level chunks)
    Case("11x2x2-20x30", 11, 2, 2, 20, 30, seed=3),
)


def identity_grids(num, L, Gh, Gw, dtype=torch.float32):
    eye = torch.eye(4, dtype=dtype)[:3].reshape(1, 12, 1, 1, 1)
    return eye.repeat(num, 1, L, Gh, Gw)


def gray_of(image):
    return GRAY[0] * image[:, 0] + GRAY[1] * image[:, 1] + GRAY[2] * image[:, 2]


def input_condition(case: Case, image64) -> bool:
    gray = gray_of(image64)
    if bool(((gray.abs() < MARGIN) | ((gray - 1).abs() < MARGIN)).any()):
        return False
    if case.L > 1:
        uz = gray[(gray > 0) & (gray < 1)] * (case.L - 1)
        if bool(((uz - uz.round()).abs() < MARGIN).any()):
            return False
    return True


def _draw(case: Case, seed: int):
    g = torch.Generator().manual_seed(seed)
    grids = identity_grids(case.num, case.L, case.Gh, case.Gw) + 0.3 * torch.randn(
        case.num, 12, case.L, case.Gh, case.Gw, generator=g)
    B = len(case.idx)
    image = torch.rand(B, 3, case.H, case.W, generator=g) * 1.4 - 0.2  # both clamps of uz are hit
    dout = torch.randn(B, 3, case.H, case.W, generator=g)
    return grids, image, dout


@functools.lru_cache(maxsize=None)
def make(case: Case):
    """(grids, image, dout) in float32: a random grid of standard deviation 0.3 around the identity, colours in
    [-0.2, 1.2], a random upstream gradient.  Shared by the tests: do not modify."""
    grids, image, dout = _draw(case, case.seed)
    assert input_condition(case, image.double()), f"{case.name}: seed {case.seed} breaks the input condition"
    return grids, image, dout


def slice_grid_sample(grids, image, idx):
    """The definition through F.grid_sample, in the dtype of its arguments."""
    B, _, H, W = image.shape
    dt = image.dtype
    x = (torch.arange(W, dtype=dt) + 0.5) / W
    y = (torch.arange(H, dtype=dt) + 0.5) / H
    coords = torch.stack([x.view(1, 1, W).expand(B, H, W), y.view(1, H, 1).expand(B, H, W), gray_of(image)], dim=-1)
    A = F.grid_sample(grids[list(idx)], ((coords - 0.5) * 2).unsqueeze(1), mode="bilinear", align_corners=True,
                      padding_mode="border")  # (B, 12, 1, H, W)
    A = A[:, :, 0].reshape(B, 3, 4, H, W)
    return (A[:, :, :3] * image[:, None]).sum(2) + A[:, :, 3]


def slice_hat(grids, image, idx):
    """The definition as the sum over lattice vertices of grid * hat(uz - l) hat(uy - j) hat(ux - i)."""
    B, _, H, W = image.shape
    _, _, L, Gh, Gw = grids.shape
    dt = image.dtype
    hat = lambda t: (1 - t.abs()).clamp(min=0)  # noqa: E731
    ux = (torch.arange(W, dtype=dt) + 0.5) / W * (Gw - 1)
    uy = (torch.arange(H, dtype=dt) + 0.5) / H * (Gh - 1)
    uz = (gray_of(image) * (L - 1)).clamp(0, L - 1)
    wx = hat(ux[None, :] - torch.arange(Gw, dtype=dt)[:, None])  # (Gw, W)
    wy = hat(uy[None, :] - torch.arange(Gh, dtype=dt)[:, None])  # (Gh, H)
    wz = hat(uz[:, None] - torch.arange(L, dtype=dt).view(1, L, 1, 1))  # (B, L, H, W)
    A = torch.einsum("bclji,blhw,jh,iw->bchw", grids[list(idx)], wz, wy, wx).reshape(B, 3, 4, H, W)
    return (A[:, :, :3] * image[:, None]).sum(2) + A[:, :, 3]


def run(fn, grids, image, dout, idx):
    """(out, dgrids, dimage) of `fn` under the upstream gradient `dout`."""
    g = grids.detach().clone().requires_grad_(True)
    x = image.detach().clone().requires_grad_(True)
    out = fn(g, x, idx)
    out.backward(dout)
    return out.detach(), g.grad, x.grad


def rel_l2(a, ref) -> float:
    a, ref = a.double().cpu(), ref.double().cpu()
    return float((a - ref).norm() / ref.norm().clamp(min=1e-300))


@functools.lru_cache(maxsize=None)
def reference(case: Case):
    """float64 (out, dgrids, dimage); the two statements of the definition must agree to 1e-12 relative."""
    grids, image, dout = (t.double() for t in make(case))
    ref = run(slice_grid_sample, grids, image, dout, case.idx)
    alt = run(slice_hat, grids, image, dout, case.idx)
    for name, a, b in zip(("out", "dgrids", "dimage"), ref, alt):
        assert rel_l2(b, a) <= 1e-12, f"{case.name}: the two statements of the definition differ in {name}"
    return ref


@functools.lru_cache(maxsize=None)
def bars(case: Case):
    """Per quantity: BAR_FACTOR times the relative L2 error of the float32 torch route against float64."""
    ref = reference(case)
    got = run(slice_grid_sample, *make(case), case.idx)
    return tuple(BAR_FACTOR * rel_l2(a, r) for a, r in zip(got, ref))


def reached_vertices(case: Case):
    """(num, Gh, Gw) bool: lattice columns with a pixel inside their support in some image of the grid (the others
    must get an exactly zero gradient)."""
    hat = lambda t: (1 - t.abs()).clamp(min=0)  # noqa: E731
    ux = (torch.arange(case.W, dtype=torch.float64) + 0.5) / case.W * (case.Gw - 1)
    uy = (torch.arange(case.H, dtype=torch.float64) + 0.5) / case.H * (case.Gh - 1)
    rx = (hat(ux[None, :] - torch.arange(case.Gw, dtype=torch.float64)[:, None]) > 0).any(1)
    ry = (hat(uy[None, :] - torch.arange(case.Gh, dtype=torch.float64)[:, None]) > 0).any(1)
    out = torch.zeros(case.num, case.Gh, case.Gw, dtype=torch.bool)
    for g in set(case.idx):
        out[g] = ry[:, None] & rx[None, :]
    return out


def tv_reference(grids):
    """The total variation of the contract, in the dtype of `grids`."""
    num = grids.shape[0]
    tv = grids.new_zeros(())
    for axis in (2, 3, 4):
        n = grids.shape[axis]
        if n > 1:
            count = grids[0].numel() // n * (n - 1)  # 12 (n - 1) (the other two sizes)
            tv = tv + grids.diff(dim=axis).pow(2).sum() / count
    return tv / num
