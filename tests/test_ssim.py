"""Fused SSIM (§8(f) next #1): the HIP kernels of csrc/gsr_ssim.hip against the float64 oracle/ssim_oracle.py, the
oracle's analytic gradient against finite differences, and the argument checks of the C entry points.  Parity unpinned
(no reference SSIM fixture, see the oracle).

Bars.  tests/ssim_cases.py holds the case table (value cases: noise, flat, near-flat, edge, black, HDR, negative, x == y;
seam cases: the extents around the 64-column / 32-row strips of the streaming forward and the 64x16 / 32x16 tiles) and
derives every bar from the error three float32 numpy restatements in different association orders make on the same
input: no bar is fitted to HIP output.  test_restatements_pass_each_others_bars holds the construction to itself on the
CPU.  Every case runs through both forward paths (ssim_stream 0 and 1) and records achieved error and bar through
tests.parity (profiles/parity_ssim.json is one run).  Achieved figures of that run, both paths, worst achieved / bar:
mean 0.27 (flat_noisy-64x128-same), per-pixel gradient 0.64 (seam-11x31-same, a borrowed bar), L2 gradient 0.40
(seam-15x65-same, a borrowed bar).  In absolute terms: noise images at every seam shape, mean <= 3.2e-7 and gradient <= 1.7e-6 of
max|grad|; flat 0.3 against 0.7, mean 3.9e-5 to 5.6e-5 and gradient 1.2e-4 to 2.2e-4 of max|grad|; flat 0.9 with 1e-3
noise, mean 1.2e-5 to 1.7e-5 and gradient 1.8e-4 (E[x^2] - mu^2 cancels against C2 = 9e-4; the fp32 restatements lose
as much).  The gradient is bitwise the same through both forward paths in every case.

Beside parity: the upstream gradient's value and sign, a requires-grad (C,H,W) input, locality (a pixel moves only the
gradient within 10 px of it, a plane only its own), no dependence on what the output buffers held before, and the
wrapper's refusal of padding="valid" images that count no pixel.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import ssim_oracle as SO
from oracle import ssim_restatements as SR
from tests import parity
from tests import ssim_cases as SC

GSR_ERR_ARG = 1


_images = SC.noise_images  # (render, gt) of (B, C, H, W, seed): uniform noise against the same noise perturbed


@pytest.mark.parametrize("padding", ["same", "valid"])
def test_oracle_gradient_finite_differences(padding):
    x, y = _images(1, 2, 19, 23, 0)
    x = x.astype(np.float64)
    _, g = SO.ssim(x, y, padding)
    rng = np.random.default_rng(1)
    for _ in range(6):
        idx = tuple(rng.integers(0, s) for s in x.shape)
        e = np.zeros_like(x)
        e[idx] = 1e-6
        fd = (SO.ssim(x + e, y, padding)[0] - SO.ssim(x - e, y, padding)[0]) / 2e-6
        assert abs(fd - g[idx]) <= 1e-6 * max(1.0, abs(g[idx])) + 1e-9


def test_identical_images_have_ssim_one():
    x, _ = _images(1, 3, 16, 16, 2)
    m, g = SO.ssim(x, x)
    assert abs(m - 1.0) < 1e-12 and np.abs(g).max() < 1e-9


# ---- the yardstick against itself (no GPU) ----
def test_case_table_covers_the_seams():
    shapes = {(c.shape[2], c.shape[3], c.padding) for c in SC.CASES if c.kind == "seam"}
    for H in SC.SEAM_H:
        for W in (11, 65, 129):
            assert (H, W, "same") in shapes and ((H, W, "valid") in shapes) == (H > 10)
    for W in SC.SEAM_W:
        for H in (11, 33):
            assert (H, W, "same") in shapes and ((H, W, "valid") in shapes) == (W > 10)
    assert {(1, 1, "same"), (1, 129, "same"), (43, 1, "same")} <= shapes
    assert all(H > 10 and W > 10 for H, W, p in shapes if p == "valid")
    assert all(c.shape[2] <= 64 and c.shape[3] <= 129 for c in SC.CASES)
    assert all(c.counted_per_plane >= SC.MIN_COUNTED for c in SC.VALUE_CASES)
    assert len(SC.VALUE_CASES) == len(SC.VALUE_GENS) * 4


def test_restatements_agree_with_the_oracle_in_float64_terms():
    """The three orders restate the oracle: on a well-conditioned image each is within fp32 rounding of it, and the
    upstream scalar multiplies the gradient."""
    case = SC.BY_NAME["noise-45x77-valid"]
    x, y = SC.inputs(case)
    ref_mean, ref_grad, T = SC.reference(case)
    assert T >= np.abs(ref_grad).max() > 0
    for order in SR.ORDERS:
        mean, grad = SR.ssim(x, y, case.padding, order=order)
        assert abs(mean - ref_mean) <= 1e-6 and np.abs(grad - ref_grad).max() <= 1e-5 * np.abs(ref_grad).max()
        _, scaled = SR.ssim(x, y, case.padding, upstream=-0.25, order=order)  # a power of two: exact
        assert np.array_equal(scaled, np.float32(-0.25) * grad)


@pytest.mark.parametrize("case", SC.VALUE_CASES, ids=lambda c: c.name)
def test_restatements_pass_each_others_bars(case):
    """Leave one out: each restatement is a correct fp32 SSIM, so it has to pass the bar built from the other two.  If
    one did not, the bar would be a coin flip for the HIP kernels as well."""
    err = SC.restatement_errors(case)
    for order in SR.ORDERS:
        bars = SC.bars_from(case, tuple(o for o in SR.ORDERS if o != order))
        for m in SC.MEASURES:
            assert err[order][m] <= bars[m], (order, m, err[order][m], bars[m])


def test_bars_catch_a_dropped_outermost_tap(monkeypatch):
    """Teeth of the seam cases, the small ones with their borrowed bars included: a restatement whose outermost window
    tap (weight 1.0e-3) is lost misses the per-pixel gradient bar of every seam case by a factor of 100 or more (163 at
    11x11 "valid" with its single counted pixel, 500 and more elsewhere).  1x1 has no neighbour for that tap to weigh and
    is left out.  The tap is lost in all six filters at every pixel, so the factor bounds from above what a tap lost
    only at one strip edge, in one filter, would show; the per-pixel measure sees such a pixel at its own error."""
    seams = [c for c in SC.CASES if c.kind == "seam" and c.shape[2:] != (1, 1)]
    bars = {c: SC.bar(c) for c in seams}  # from the true window
    lost = SR.window()
    lost[0] = 0
    monkeypatch.setattr(SR, "window", lambda: lost)
    for c in seams:
        x, y = SC.inputs(c)
        ref_mean, ref_grad, _ = SC.reference(c)
        err = SC.errors(*SR.ssim(x, y, c.padding), ref_mean, ref_grad)
        assert err["grad_max"] >= 100 * bars[c]["grad_max"], (c.name, err["grad_max"], bars[c]["grad_max"])


# ---- argument checks of the C entry points (the library loads without a device) ----
class _Buffers:
    """n floats per pointer.  Device memory where there is a device, so that a check that stopped refusing would launch
    on real memory; host memory otherwise (never dereferenced: every call here is refused before device work)."""

    def __init__(self, n, count):
        if torch.cuda.is_available():
            self.keep = [torch.zeros(n, device="cuda") for _ in range(count)]
            self.ptr = [t.data_ptr() for t in self.keep]
        else:
            self.keep = [(ctypes.c_float * n)() for _ in range(count)]
            self.ptr = [ctypes.addressof(b) for b in self.keep]


@pytest.mark.parametrize("H,W", [(5, 5), (10, 10), (10, 40), (40, 10)])
def test_valid_padding_refuses_images_that_count_no_pixel(H, W):
    """(H - 10) * (W - 10) is positive when both extents are below 10: the count's sign does not say that no pixel is
    counted.  Both entry points refuse unless H > 10 and W > 10."""
    from gaussian_splatting_lightning_amd import _native
    lib = _native.load()
    b = _Buffers(2 * H * W, 8)
    p = b.ptr
    assert lib.gsr_ssim_forward(2, H, W, p[0], p[1], 1, p[2], None, None, None, None) == GSR_ERR_ARG
    assert b"ssim" in lib.gsr_last_error() and b"valid" in lib.gsr_last_error()
    assert lib.gsr_ssim_forward(2, H, W, p[0], p[1], 1, p[2], p[3], p[4], p[5], None) == GSR_ERR_ARG
    assert b"ssim" in lib.gsr_last_error() and b"valid" in lib.gsr_last_error()
    assert lib.gsr_ssim_backward(2, H, W, p[0], p[1], 1, p[6], p[3], p[4], p[5], p[7], None) == GSR_ERR_ARG
    assert b"ssim" in lib.gsr_last_error() and b"valid" in lib.gsr_last_error()


def test_ssim_abi_argument_validation_without_device():
    from gaussian_splatting_lightning_amd import _native
    lib = _native.load()
    # sizes: refused before any pointer is looked at
    # (2 * 32768 * 32768 = 2^31 is one past the largest element count the kernels index)
    for planes, H, W, what in [(65536, 11, 11, b"planes"), (2, 32768, 32768, b"large"), (65535, 1024, 1024, b"large"),
                               (0, 11, 11, b"empty"), (1, 0, 11, b"empty"), (1, 11, -3, b"empty")]:
        assert lib.gsr_ssim_forward(planes, H, W, None, None, 0, None, None, None, None, None) == GSR_ERR_ARG
        assert b"ssim" in lib.gsr_last_error() and what in lib.gsr_last_error()
        assert lib.gsr_ssim_backward(planes, H, W, None, None, 0, None, None, None, None, None, None) == GSR_ERR_ARG
        assert b"ssim" in lib.gsr_last_error() and what in lib.gsr_last_error()
    assert lib.gsr_ssim_num_partials(0, 11, 11) == 0 and lib.gsr_ssim_num_partials(1, 11, 11) >= 1
    # pointers: a missing image or output, and derivative maps that are neither all given nor all NULL
    b = _Buffers(2 * 11 * 11, 8)
    p = b.ptr
    assert lib.gsr_ssim_forward(2, 11, 11, None, p[1], 0, p[2], None, None, None, None) == GSR_ERR_ARG
    assert b"ssim" in lib.gsr_last_error() and b"null" in lib.gsr_last_error()
    assert lib.gsr_ssim_forward(2, 11, 11, p[0], p[1], 0, None, None, None, None, None) == GSR_ERR_ARG
    for maps in [(p[3], None, None), (None, p[4], None), (None, None, p[5]), (p[3], p[4], None), (p[3], None, p[5]),
                 (None, p[4], p[5])]:
        assert lib.gsr_ssim_forward(2, 11, 11, p[0], p[1], 0, p[2], *maps, None) == GSR_ERR_ARG
        assert b"ssim" in lib.gsr_last_error() and b"derivative maps" in lib.gsr_last_error()
        assert lib.gsr_ssim_backward(2, 11, 11, p[0], p[1], 0, p[6], *maps, p[7], None) == GSR_ERR_ARG
        assert b"ssim" in lib.gsr_last_error() and b"null" in lib.gsr_last_error()


def test_wrapper_checks_padding_before_anything_else():
    from fused_ssim import fused_ssim
    x = torch.zeros(1, 1, 5, 5)
    with pytest.raises(ValueError, match="padding"):
        fused_ssim(x, x, padding="full")


# ---- the HIP kernels ----
def _run(x, y, padding, dev, upstream=1.0):
    """(mean, upstream * dmean/dimg1) of the HIP path as a float and a numpy array of x's shape."""
    from fused_ssim import fused_ssim
    xt = torch.tensor(x, device=dev, requires_grad=True)
    m = fused_ssim(xt, torch.tensor(y, device=dev), padding=padding)
    (upstream * m).backward()
    return float(m.detach()), xt.grad.cpu().numpy()


MODES = ((0, "tiled"), (1, "stream"))  # ssim_stream: the tiled forward, the streaming forward (the default)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,padding", [((1, 3, 100, 150), "same"), ((2, 3, 67, 45), "valid"),
                                           ((1, 1, 11, 11), "same"), ((1, 3, 1080, 1920), "same")])
def test_fused_ssim_matches_oracle(gpu_device, shape, padding):
    from fused_ssim import fused_ssim
    x, y = _images(*shape, seed=3)
    ref_m, ref_g = SO.ssim(x, y, padding)
    xt = torch.tensor(x, device=gpu_device, requires_grad=True)
    m = fused_ssim(xt, torch.tensor(y, device=gpu_device), padding=padding)
    (1 - m).backward()
    assert abs(float(m) - ref_m) <= 2e-6
    got = -xt.grad.cpu().numpy()
    err = np.abs(got - ref_g).max() / np.abs(ref_g).max()
    assert err <= 1e-4, err


@pytest.mark.gpu
def test_fused_ssim_eval_mode_and_3d_input(gpu_device):
    from fused_ssim import fused_ssim
    x, y = _images(1, 3, 40, 52, 4)
    a = fused_ssim(torch.tensor(x[0], device=gpu_device), torch.tensor(y[0], device=gpu_device), train=False)
    assert abs(float(a) - SO.ssim(x, y)[0]) <= 2e-6


@pytest.mark.gpu
@pytest.mark.parametrize("shape,padding", [((1, 3, 100, 150), "same"), ((2, 3, 67, 45), "valid"),
                                           ((1, 1, 11, 11), "same"), ((1, 3, 1080, 1920), "same")])
def test_streaming_ssim_matches_tiled_kernels(gpu_device, shape, padding):
    """The streaming forward (one wave per 64-column x 32-row strip, rows walked once) forms every filter sum in the
    tiled kernel's order: the derivative maps, hence the gradient, are bitwise the tiled ones and the mean equal up
    to the grouping of its partial sums."""
    from fused_ssim import fused_ssim
    from gaussian_splatting_lightning_amd import _native
    x, y = _images(*shape, seed=5)
    out = {}
    for mode in (0, 1):  # tiled forward, streaming forward (the default)
        with _native.tuned(ssim_stream=mode):
            xt = torch.tensor(x, device=gpu_device, requires_grad=True)
            m = fused_ssim(xt, torch.tensor(y, device=gpu_device), padding=padding)
            (1 - m).backward()
            out[mode] = (float(m), xt.grad.cpu().numpy())
    assert abs(out[0][0] - out[1][0]) <= 1e-6 * max(1.0, abs(out[0][0]))
    assert np.array_equal(out[0][1], out[1][1])


@pytest.fixture(params=MODES, ids=lambda m: m[1])
def forward_path(request, gpu_device):
    """Runs the test once through each forward."""
    from gaussian_splatting_lightning_amd import _native
    with _native.tuned(ssim_stream=request.param[0]):
        yield request.param[1]


def _sig(v):
    return float(f"{v:.4g}")


def _worst_pixel(got, ref):
    d = np.abs(np.asarray(got, np.float64) - ref)
    idx = np.unravel_index(int(d.argmax()), d.shape)
    return [int(i) for i in idx]


@pytest.mark.gpu
@pytest.mark.parametrize("case", SC.CASES, ids=lambda c: c.name)
def test_parity_with_oracle_under_derived_bars(gpu_device, case):
    """Mean, per-pixel gradient and L2 gradient error of both forward paths against the float64 oracle under
    SC.bar(case).  The record keeps four digits of each achieved error and bar."""
    from gaussian_splatting_lightning_amd import _native
    x, y = SC.inputs(case)
    ref_mean, ref_grad, _ = SC.reference(case)
    bars = SC.bar(case)
    err, grads = {}, {}
    for mode, name in MODES:
        with _native.tuned(ssim_stream=mode):
            mean, grads[name] = _run(x, y, case.padding, gpu_device)
        assert np.isfinite(mean) and np.isfinite(grads[name]).all()
        err[name] = SC.errors(mean, grads[name], ref_mean, ref_grad)
    assert np.array_equal(grads["tiled"], grads["stream"])  # the two forwards form every sum in the same order
    rec = {"bar": {m: _sig(bars[m]) for m in SC.MEASURES}}
    rec.update({name: {m: _sig(err[name][m]) for m in SC.MEASURES} for _, name in MODES})
    parity.record(case.name, "ssim", rec)
    print(case.name, err, bars, "worst pixel", _worst_pixel(grads["stream"], ref_grad))
    for _, name in MODES:
        for m in SC.MEASURES:
            assert err[name][m] <= bars[m], (name, m, err[name][m], bars[m])


UPSTREAM_SHAPE = (1, 2, 33, 65)


@pytest.mark.gpu
@pytest.mark.parametrize("padding", ["same", "valid"])
@pytest.mark.parametrize("upstream", [-1.0, 0.2, -0.2, 3.0])
def test_upstream_gradient_scales_the_result(gpu_device, padding, upstream, forward_path):
    """dL/dimg1 = dL/dmean * dmean/dimg1, in value and sign: the bar is the case's bar times |dL/dmean|."""
    case = SC.BY_NAME[f"seam-33x65-{padding}"]
    assert case.shape == UPSTREAM_SHAPE and case.counted_per_plane >= SC.MIN_COUNTED
    x, y = SC.inputs(case)
    ref_mean, ref_grad, _ = SC.reference(case)
    bars = SC.bar(case, upstream)
    mean, grad = _run(x, y, padding, gpu_device, upstream=upstream)
    err = SC.errors(mean, grad, ref_mean, upstream * ref_grad)
    parity.record(f"{case.name}-upstream{upstream:+g}", f"ssim-{forward_path}",
                  {"bar": {m: _sig(bars[m]) for m in SC.MEASURES}, "err": {m: _sig(err[m]) for m in SC.MEASURES}})
    for m in SC.MEASURES:
        assert err[m] <= bars[m], (m, err[m], bars[m])
    assert np.abs(grad).max() >= 0.5 * abs(upstream) * np.abs(ref_grad).max()


@pytest.mark.gpu
@pytest.mark.parametrize("padding", ["same", "valid"])
def test_zero_upstream_gradient_gives_exact_zeros(gpu_device, padding, forward_path):
    x, y = SC.inputs(SC.BY_NAME[f"seam-33x65-{padding}"])
    _, grad = _run(x, y, padding, gpu_device, upstream=0.0)
    assert grad.shape == x.shape and np.all(grad == 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("padding", ["same", "valid"])
def test_requires_grad_3d_input_matches_4d_call(gpu_device, padding, forward_path):
    from fused_ssim import fused_ssim
    x, y = SC.inputs(SC.BY_NAME[f"seam-33x65-{padding}"])
    mean4, grad4 = _run(x, y, padding, gpu_device, upstream=-0.2)
    x3 = torch.tensor(x[0], device=gpu_device, requires_grad=True)
    m = fused_ssim(x3, torch.tensor(y[0], device=gpu_device), padding=padding)
    (-0.2 * m).backward()
    assert x3.grad.shape == x3.shape == (2, 33, 65)
    assert float(m.detach()) == mean4 and np.array_equal(x3.grad.cpu().numpy(), grad4[0])


LOCALITY_PIXELS = [(0, 0), (31, 63), (32, 64), (16, 32), (42, 74), (21, 37)]


@pytest.mark.gpu
@pytest.mark.parametrize("padding", ["same", "valid"])
def test_gradient_is_local_to_a_changed_pixel(gpu_device, padding):
    """A pixel of img1 reaches the SSIM map within 5 px and the map reaches the gradient within 5 px: every gradient
    entry farther than 10 px (Chebyshev) from a changed pixel, and every entry of the other plane, is bitwise
    unchanged.  No tolerance: a tile or strip that read a neighbour's halo wrongly would move entries outside."""
    from gaussian_splatting_lightning_amd import _native
    H, W = 43, 75
    x, y = SC.noise_images(1, 2, H, W, seed=11)
    rows, cols = np.mgrid[0:H, 0:W]
    for mode, _ in MODES:
        with _native.tuned(ssim_stream=mode):
            _, base = _run(x, y, padding, gpu_device)
            for py, px in LOCALITY_PIXELS:
                x2 = x.copy()
                x2[0, 0, py, px] = 1.0 - x2[0, 0, py, px]
                assert abs(x2[0, 0, py, px] - x[0, 0, py, px]) > 1e-3
                _, moved = _run(x2, y, padding, gpu_device)
                near = np.maximum(np.abs(rows - py), np.abs(cols - px)) <= 10
                changed = moved != base
                assert not changed[0, 1].any(), (mode, py, px)
                assert not (changed[0, 0] & ~near).any(), (mode, py, px, np.argwhere(changed[0, 0] & ~near)[:4])
                assert (changed[0, 0] & near).any(), (mode, py, px)


@pytest.mark.gpu
@pytest.mark.parametrize("padding", ["same", "valid"])
def test_planes_are_independent(gpu_device, padding, forward_path):
    x, y = SC.inputs(SC.BY_NAME[f"seam-planes2x3-33x65-{padding}"])
    x2 = x.copy()
    x2[0, 0] = 1.0 - x2[0, 0]
    _, base = _run(x, y, padding, gpu_device)
    _, moved = _run(x2, y, padding, gpu_device)
    base, moved = base.reshape(6, 33, 65), moved.reshape(6, 33, 65)
    assert np.array_equal(base[1:], moved[1:]) and not np.array_equal(base[0], moved[0])


@pytest.mark.gpu
@pytest.mark.parametrize("padding", ["same", "valid"])
def test_result_does_not_depend_on_stale_buffer_contents(gpu_device, padding):
    """The partial sums, the three derivative maps and dx come from torch.empty.  With the inputs already allocated,
    fill freed blocks of exactly those sizes with NaN, so that the allocator hands them out next: the result has to be
    finite and bitwise the unpoisoned one.  (Which block the allocator hands out is its business; the test below does
    the same on buffers it fills itself.)"""
    from fused_ssim import fused_ssim
    from gaussian_splatting_lightning_amd import _native
    x, y = SC.inputs(SC.BY_NAME[f"seam-33x65-{padding}"])
    lib = _native.load()
    yt = torch.tensor(y, device=gpu_device)

    def run(poison):
        xt = torch.tensor(x, device=gpu_device, requires_grad=True)
        if poison:
            sizes = [lib.gsr_ssim_num_partials(2, 33, 65)] + [x.size] * 4
            blocks = [torch.full((n,), float("nan"), device=gpu_device) for n in sizes]
            torch.cuda.synchronize()
            del blocks
        m = fused_ssim(xt, yt, padding=padding)
        m.backward()
        return float(m.detach()), xt.grad.cpu().numpy()

    for mode, _ in MODES:
        with _native.tuned(ssim_stream=mode):
            clean, got = run(False), run(True)
        assert np.isfinite(got[0]) and np.isfinite(got[1]).all()
        assert got[0] == clean[0] and np.array_equal(got[1], clean[1])


@pytest.mark.gpu
@pytest.mark.parametrize("padding", ["same", "valid"])
def test_kernels_overwrite_nan_filled_outputs(gpu_device, padding, forward_path):
    """The C entry points on output buffers filled with NaN beforehand: every partial sum, every element of the three
    maps and of dx is written, and the result is bitwise the wrapper's."""
    from gaussian_splatting_lightning_amd import _native
    from gaussian_splatting_lightning_amd.rasterizer import _stream_handle
    case = SC.BY_NAME[f"seam-33x65-{padding}"]
    x, y = SC.inputs(case)
    mean, grad = _run(x, y, padding, gpu_device)
    lib = _native.load()
    planes, H, W = 2, 33, 65
    valid = int(padding == "valid")
    xt, yt = torch.tensor(x, device=gpu_device), torch.tensor(y, device=gpu_device)
    nan = float("nan")
    partial = torch.full((lib.gsr_ssim_num_partials(planes, H, W),), nan, device=gpu_device)
    maps = [torch.full_like(xt, nan) for _ in range(3)]
    dx = torch.full_like(xt, nan)
    one = torch.ones(1, device=gpu_device)
    stream = _stream_handle(gpu_device)
    _native.check(lib.gsr_ssim_forward(planes, H, W, xt.data_ptr(), yt.data_ptr(), valid, partial.data_ptr(),
                                       maps[0].data_ptr(), maps[1].data_ptr(), maps[2].data_ptr(), stream), "forward")
    _native.check(lib.gsr_ssim_backward(planes, H, W, xt.data_ptr(), yt.data_ptr(), valid, one.data_ptr(),
                                        maps[0].data_ptr(), maps[1].data_ptr(), maps[2].data_ptr(), dx.data_ptr(),
                                        stream), "backward")
    torch.cuda.synchronize()
    for t in [partial, dx] + maps:
        assert bool(torch.isfinite(t).all())
    assert float(partial.sum() / (planes * case.counted_per_plane)) == mean
    assert np.array_equal(dx.cpu().numpy(), grad)


@pytest.mark.gpu
def test_wrapper_valid_padding_size_check(gpu_device, forward_path):
    """padding="valid" needs H > 10 and W > 10; 11x11 counts exactly one pixel per plane."""
    from fused_ssim import fused_ssim
    for H, W in [(5, 5), (10, 40)]:
        t = torch.rand(1, 2, H, W, device=gpu_device, requires_grad=True)
        with pytest.raises(RuntimeError, match="smaller than the SSIM window"):
            fused_ssim(t, torch.rand(1, 2, H, W, device=gpu_device), padding="valid")
    case = SC.BY_NAME["seam-11x11-valid"]
    assert case.counted_per_plane == 1
    x, y = SC.inputs(case)
    ref_mean, ref_grad, _ = SC.reference(case)
    mean, grad = _run(x, y, "valid", gpu_device)
    err, bars = SC.errors(mean, grad, ref_mean, ref_grad), SC.bar(case)
    for m in SC.MEASURES:
        assert err[m] <= bars[m], (m, err[m], bars[m])
