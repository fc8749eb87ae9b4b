"""Bilateral-grid slice, gradients and total variation on the GPU (csrc/gsr_bilagrid.hip) against the float64
reference of tests/bilagrid_cases.py.

Cases (L x Gh x Gw, H x W) and what each reaches:
  8x16x16, 37x53          odd sizes; rows shorter than a wave; a 64x16 tile spans 144 lattice columns, over the LDS
                          budget, so this and the next case take the slice's global-memory path (the others: LDS)
  8x16x16, 5x7            a lattice far finer than the image: 116 of its 256 columns see no pixel (exact zeros)
  1x1x1, 4x4              the exposure-matrix case, every axis of size 1
  3x1x5, 9x130            a size-1 axis among others; rows that straddle a wave; 4-level accumulators
  2x2x3, 40x300           cells wider than a wave (150 px); the support split over 11 workgroups and summed in order
  8x16x16, 64x96, B = 3   idx = [2, 0, 2] of num = 4: a batch, a grid named twice, grids 1 and 3 exactly zero
  11x2x2, 20x30           two level chunks (L > 8) in the grid gradient

Bars.  Per case and quantity (output, dgrids, dimage) the bar is 4 x the relative L2 error the float32 torch route
(F.grid_sample on the CPU) makes against float64 on the same input, BC.bars(); nothing is fitted to HIP output, and
by the input condition of BC.make() no pixel is excluded.  Achieved errors and bars are recorded through tests.parity.
The identity grid returns the image bit for bit (the interpolation is a chain of lerps a + f (b - a), exact on a
constant grid, and 1 * v + 0 + 0 + 0 is exact), asserted with torch.equal.
"""
import ctypes
import functools

import pytest
import torch

from gaussian_splatting_lightning_amd import BilateralGrid, _native, slice_image, total_variation_loss
from tests import bilagrid_cases as BC
from tests import parity

pytestmark = pytest.mark.gpu


def _hip(case, dev):
    grids, image, dout = (t.to(dev) for t in BC.make(case))
    return BC.run(lambda g, x, idx: slice_image(g, x, list(idx)), grids, image, dout, case.idx)


@functools.lru_cache(maxsize=None)
def _hip_cached(case, dev):
    return _hip(case, dev)


@pytest.mark.parametrize("case", BC.CASES, ids=lambda c: c.name)
def test_slice_forward_backward_parity(gpu_device, case):
    ref, bars = BC.reference(case), BC.bars(case)
    got = _hip_cached(case, gpu_device)
    errs = [BC.rel_l2(a, r) for a, r in zip(got, ref)]
    record = {k: {"rel_l2": e, "bar": b} for k, e, b in zip(("out", "dgrids", "dimage"), errs, bars)}
    print(case.name, record)
    parity.record(f"bilagrid-{case.name}", "slice", record)
    dg = got[1].cpu()
    unreached = ~BC.reached_vertices(case)[:, None, None].expand_as(dg)
    assert bool((dg[unreached] == 0).all()), "a vertex no pixel reaches must get an exactly zero gradient"
    for g in set(range(case.num)) - set(case.idx):
        assert bool((dg[g] == 0).all()), f"grid {g} is selected by no image"
    for name, e, b in zip(("out", "dgrids", "dimage"), errs, bars):
        assert e <= b, f"{case.name} {name}: rel L2 {e:.3e} above the bar {b:.3e}"


@pytest.mark.parametrize("shape", [(8, 16, 16, 37, 53), (1, 1, 1, 4, 4), (8, 16, 16, 5, 7), (3, 1, 5, 9, 130)])
def test_identity_grid_returns_the_image_bit_for_bit(gpu_device, shape):
    L, Gh, Gw, H, W = shape
    g = torch.Generator().manual_seed(5)
    image = (torch.rand(2, 3, H, W, generator=g) * 1.4 - 0.2).to(gpu_device)
    out = slice_image(BC.identity_grids(2, L, Gh, Gw).to(gpu_device), image, [1, 0])
    assert torch.equal(out, image)


@pytest.mark.parametrize("case", [BC.CASES[4], BC.CASES[5]], ids=lambda c: c.name)
def test_backward_is_deterministic(gpu_device, case):
    a, b = _hip_cached(case, gpu_device), _hip(case, gpu_device)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_flat_image_on_a_level(gpu_device):
    """gray = 0.5 with L = 9: uz = 4 sits on a lattice level.  Forward only (either one-sided derivative is allowed
    there); the output is continuous across the level, so the bar is built as everywhere else."""
    g = torch.Generator().manual_seed(9)
    grids = BC.identity_grids(1, 9, 4, 5) + 0.3 * torch.randn(1, 12, 9, 4, 5, generator=g)
    image = torch.full((1, 3, 21, 70), 0.5)
    ref = BC.slice_grid_sample(grids.double(), image.double(), (0,))
    bar = BC.BAR_FACTOR * BC.rel_l2(BC.slice_grid_sample(grids, image, (0,)), ref)
    err = BC.rel_l2(slice_image(grids.to(gpu_device), image.to(gpu_device), 0), ref)
    print("flat", err, bar)
    parity.record("bilagrid-flat-9x4x5-21x70", "slice", {"out": {"rel_l2": err, "bar": bar}})
    assert 0 < bar and err <= bar


@pytest.mark.parametrize("case", [BC.CASES[4], BC.CASES[5]], ids=lambda c: c.name)
def test_backward_overwrites_prefilled_outputs(gpu_device, case):
    """The C entry point writes every element of both gradients, and reads nothing it did not write from the
    workspace: buffers pre-filled with NaN come back as the autograd result."""
    lib = _native.load()
    grids, image, dout = (t.to(gpu_device) for t in BC.make(case))
    num, _, L, Gh, Gw = grids.shape
    B, _, H, W = image.shape
    dg, dx = torch.full_like(grids, float("nan")), torch.full_like(image, float("nan"))
    nbytes = lib.gsr_bilagrid_workspace_bytes(L, Gh, Gw, H, W)
    assert (nbytes > 0) == (case is BC.CASES[4])
    ws = torch.full((max(nbytes // 4, 1),), float("nan"), device=gpu_device)
    idx = (ctypes.c_int32 * B)(*case.idx)
    rc = lib.gsr_bilagrid_slice_backward(num, L, Gh, Gw, grids.data_ptr(), B, H, W, image.data_ptr(), idx,
                                         dout.data_ptr(), dg.data_ptr(), dx.data_ptr(), ws.data_ptr(),
                                         torch.cuda.current_stream(gpu_device).cuda_stream)
    _native.check(rc, "bilagrid slice backward")
    assert not bool(torch.isnan(dg).any()) and not bool(torch.isnan(dx).any())
    _, want_dg, want_dx = _hip_cached(case, gpu_device)
    assert torch.equal(dg, want_dg) and torch.equal(dx, want_dx)


def test_index_forms_and_layouts_agree(gpu_device):
    case = BC.CASES[5]
    grids, image, _ = (t.to(gpu_device) for t in BC.make(case))
    want = _hip_cached(case, gpu_device)[0]
    assert torch.equal(slice_image(grids, image, torch.tensor(case.idx)), want)
    assert torch.equal(slice_image(grids, image, torch.tensor(case.idx, device=gpu_device)), want)
    assert torch.equal(slice_image(grids, image[1], 0), want[1])  # (3, H, W) with an int
    nc = image.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)  # same values, not contiguous
    assert not nc.is_contiguous() and torch.equal(slice_image(grids, nc, list(case.idx)), want)
    x = image[:1].clone().requires_grad_(True)  # the image gradient alone
    slice_image(grids, x, [2]).sum().backward()
    assert x.grad is not None and bool(torch.isfinite(x.grad).all())


def test_total_variation(gpu_device):
    """Value: relative error at most 32 * 2^-24 (three roundings per term -- difference, square, scale -- and at most
    about 25 additions deep: 8 per thread, 6 + 2 across the workgroup, the caller's sum of 36 partials).  Gradient:
    4 x the relative L2 error of float32 torch autograd against float64, as for the slice."""
    g = torch.Generator().manual_seed(3)
    grids = BC.identity_grids(3, 8, 16, 16) + 0.3 * torch.randn(3, 12, 8, 16, 16, generator=g)
    up = 0.7

    def route(x, fn):
        x = x.detach().clone().requires_grad_(True)
        tv = fn(x)
        (up * tv).backward()
        return tv.detach(), x.grad

    tv64, dg64 = route(grids.double(), BC.tv_reference)
    _, dg32 = route(grids, BC.tv_reference)
    tv, dg = route(grids.to(gpu_device), total_variation_loss)
    err_v, err_g, bar_g = abs(float(tv) - float(tv64)) / float(tv64), BC.rel_l2(dg, dg64), 4 * BC.rel_l2(dg32, dg64)
    print("tv", err_v, err_g, bar_g)
    parity.record("bilagrid-tv-3x8x16x16", "tv", {"value": {"rel": err_v, "bar": 32 * 2.0 ** -24},
                                                  "dgrids": {"rel_l2": err_g, "bar": bar_g}})
    assert err_v <= 32 * 2.0 ** -24
    assert err_g <= bar_g
    # 1x1x1: no differences at all -- exactly 0, with an exactly zero gradient
    one = (torch.randn(5, 12, 1, 1, 1, generator=g)).to(gpu_device)
    tv, dg = route(one, total_variation_loss)
    assert float(tv) == 0.0 and bool((dg == 0).all())
    # mixed size-1 axes against float64
    mixed = torch.randn(2, 12, 3, 1, 5, generator=g)
    tv, dg = route(mixed.to(gpu_device), total_variation_loss)
    tv64, dg64 = route(mixed.double(), BC.tv_reference)
    assert abs(float(tv) - float(tv64)) <= 32 * 2.0 ** -24 * float(tv64)
    assert BC.rel_l2(dg, dg64) <= 4 * BC.rel_l2(route(mixed, BC.tv_reference)[1], dg64)


def test_module_adam_step_lowers_the_loss(gpu_device):
    g = torch.Generator().manual_seed(4)
    image = torch.rand(2, 3, 24, 40, generator=g).to(gpu_device)
    gain = torch.tensor([1.2, 0.9, 0.8], device=gpu_device).view(1, 3, 1, 1)
    target = image * gain + 0.05  # an exposure / white-balance shift
    bg = BilateralGrid(3, grid_X=4, grid_Y=4, grid_W=2).to(gpu_device)
    opt = torch.optim.Adam(bg.parameters(), lr=1e-2)

    def l1():
        return (bg(image, [2, 0]) - target).abs().mean()

    before = l1()
    (before + 10 * bg.tv_loss()).backward()
    assert bool((bg.grids.grad[1] == 0).all())  # grid 1 saw no image and the identity has no variation
    assert bool((bg.grids.grad[0] != 0).any()) and bool((bg.grids.grad[2] != 0).any())
    opt.step()
    with torch.no_grad():
        after = l1()
    assert float(after) < float(before.detach())
