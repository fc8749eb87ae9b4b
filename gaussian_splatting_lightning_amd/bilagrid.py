"""Per-image bilateral-grid colour correction on the HIP kernels of csrc/gsr_bilagrid.hip.

A bilateral grid (Wang et al., "Bilateral Guided Radiance Field Processing", SIGGRAPH 2024; gsplat's `lib_bilagrid`)
is a small 3-D lattice of 3x4 affine colour transforms indexed by pixel position and luma.  The rendered image is
sliced through its view's grid before the loss, which absorbs per-image exposure, white balance and tone, and a
total-variation term keeps the grid smooth:

    bg = BilateralGrid(num_views)
    image = render(...)                                  # (3, H, W)
    loss = photometric(bg(image, view_idx), gt) + 10 * bg.tv_loss()

Evaluation uses the un-sliced render.  `grids` is (num, 12, L, Gh, Gw) fp32, gsplat's layout: channel 4r + k
multiplies input colour k (k = 3: the offset) into output colour r; the official 3DGS per-image exposure matrix is the
1x1x1 grid.  The definition (include/gsrast.h) is `F.grid_sample(mode="bilinear", align_corners=True,
padding_mode="border")` at ((x, y, gray) - 0.5) * 2 over pixel centres.  The gradient to `grids` is a fixed-order
gather: two calls give the same bits.  No CPU fallback: the HIP library must load.
"""
from __future__ import annotations

import ctypes

import torch

from . import _native
from .rasterizer import _stream_handle

__all__ = ["BilateralGrid", "slice_image", "total_variation_loss"]


def _check_grids(grids) -> None:
    if not isinstance(grids, torch.Tensor) or grids.dim() != 5 or grids.shape[1] != 12:
        shape = tuple(grids.shape) if isinstance(grids, torch.Tensor) else type(grids).__name__
        raise RuntimeError(f"grids must be (num, 12, L, Gh, Gw), got {shape}")
    if grids.dtype != torch.float32:
        raise RuntimeError(f"grids must be float32, got {grids.dtype} for shape {tuple(grids.shape)}")
    if min(grids.shape) == 0:
        raise RuntimeError(f"empty grids {tuple(grids.shape)}")


def _check_device(t: torch.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be on a HIP device, got {t.device}: there is no CPU path")


def _indices(idx, B: int, num: int) -> list:
    if isinstance(idx, torch.Tensor):
        if idx.dim() > 1 or idx.dtype.is_floating_point or idx.dtype == torch.bool:
            raise RuntimeError(f"idx must be an int, a list or an integer tensor of length {B}, got "
                               f"{idx.dtype} {tuple(idx.shape)}")
        idx = idx.detach().reshape(-1).tolist()  # (a device tensor is read back: the C entry points take host indices)
    elif isinstance(idx, int):
        idx = [idx]
    else:
        idx = [int(i) for i in idx]
    if len(idx) != B:
        raise ValueError(f"idx has {len(idx)} entries for a batch of {B} images")
    for i in idx:
        if not 0 <= i < num:
            raise ValueError(f"grid index {i} outside [0, {num}) of grids")
    return idx


class _Slice(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grids, image, idx):
        lib = _native.load()
        g = grids.detach().contiguous()
        x = image.detach()
        if x.dtype != torch.float32:
            x = x.float()
        x = x.contiguous()
        num, _, L, Gh, Gw = g.shape
        B, _, H, W = x.shape
        c_idx = (ctypes.c_int32 * B)(*idx)
        out = torch.empty_like(x)
        rc = lib.gsr_bilagrid_slice_forward(num, L, Gh, Gw, g.data_ptr(), B, H, W, x.data_ptr(), c_idx, out.data_ptr(),
                                            _stream_handle(x.device))
        _native.check(rc, "bilagrid slice")
        ctx.save_for_backward(g, x)
        ctx.idx, ctx.image_dtype = c_idx, image.dtype
        return out

    @staticmethod
    def backward(ctx, dout):
        g, x = ctx.saved_tensors
        lib = _native.load()
        num, _, L, Gh, Gw = g.shape
        B, _, H, W = x.shape
        go = dout.detach().float().contiguous()
        dg = torch.empty_like(g) if ctx.needs_input_grad[0] else None
        dx = torch.empty_like(x) if ctx.needs_input_grad[1] else None
        ws = None
        if dg is not None:
            nbytes = lib.gsr_bilagrid_workspace_bytes(L, Gh, Gw, H, W)
            ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device) if nbytes else None
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        rc = lib.gsr_bilagrid_slice_backward(num, L, Gh, Gw, g.data_ptr(), B, H, W, x.data_ptr(), ctx.idx,
                                             go.data_ptr(), ptr(dg), ptr(dx), ptr(ws), _stream_handle(x.device))
        _native.check(rc, "bilagrid slice backward")
        if dx is not None and dx.dtype != ctx.image_dtype:
            dx = dx.to(ctx.image_dtype)
        return dg, dx, None


def slice_image(grids: torch.Tensor, image: torch.Tensor, idx) -> torch.Tensor:
    """`image` (3, H, W) or (B, 3, H, W), sliced through `grids[idx]` ((num, 12, L, Gh, Gw) fp32); `idx` is an int, a
    list or a CPU / GPU integer tensor with one grid index per image.  Differentiable w.r.t. `grids` and `image`."""
    _check_grids(grids)
    if not isinstance(image, torch.Tensor) or image.dim() not in (3, 4) or image.shape[-3] != 3:
        shape = tuple(image.shape) if isinstance(image, torch.Tensor) else type(image).__name__
        raise RuntimeError(f"image must be (3, H, W) or (B, 3, H, W), got {shape}")
    batched = image.dim() == 4
    x = image if batched else image.unsqueeze(0)
    if x.numel() == 0:
        raise RuntimeError(f"empty image {tuple(image.shape)}")
    indices = _indices(idx, x.shape[0], grids.shape[0])
    _check_device(grids, "grids")
    _check_device(x, "image")
    if x.device != grids.device:
        raise RuntimeError(f"grids on {grids.device} and image on {x.device}")
    out = _Slice.apply(grids, x, indices)
    return out if batched else out.squeeze(0)


class _TotalVariation(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grids):
        lib = _native.load()
        g = grids.detach().contiguous()
        num, _, L, Gh, Gw = g.shape
        partial = torch.empty(lib.gsr_bilagrid_tv_num_partials(num, L, Gh, Gw), dtype=torch.float32, device=g.device)
        rc = lib.gsr_bilagrid_tv_forward(num, L, Gh, Gw, g.data_ptr(), partial.data_ptr(), _stream_handle(g.device))
        _native.check(rc, "bilagrid tv")
        ctx.save_for_backward(g)
        return partial.sum()

    @staticmethod
    def backward(ctx, grad):
        g, = ctx.saved_tensors
        lib = _native.load()
        num, _, L, Gh, Gw = g.shape
        d = grad.detach().float().reshape(1).contiguous()
        dg = torch.empty_like(g)
        rc = lib.gsr_bilagrid_tv_backward(num, L, Gh, Gw, g.data_ptr(), d.data_ptr(), dg.data_ptr(),
                                          _stream_handle(g.device))
        _native.check(rc, "bilagrid tv backward")
        return dg


def total_variation_loss(grids: torch.Tensor) -> torch.Tensor:
    """gsplat's `total_variation_loss`: per lattice axis the mean squared first difference (sum over all grids divided
    by the count of differences in one grid, 0 for an axis of size 1), summed over the axes and divided by `num`."""
    _check_grids(grids)
    _check_device(grids, "grids")
    return _TotalVariation.apply(grids)


class BilateralGrid(torch.nn.Module):
    """`num` identity-initialised bilateral grids of `grid_X` x `grid_Y` vertices over the image and `grid_W` luma
    levels (gsplat's `BilateralGrid` constructor and `grids` layout)."""

    def __init__(self, num: int, grid_X: int = 16, grid_Y: int = 16, grid_W: int = 8):
        super().__init__()
        if min(num, grid_X, grid_Y, grid_W) <= 0:
            raise ValueError(f"num and the grid sizes must be positive, got {(num, grid_X, grid_Y, grid_W)}")
        self.grid_width, self.grid_height, self.grid_guidance = grid_X, grid_Y, grid_W
        eye = torch.eye(4, dtype=torch.float32)[:3].reshape(12)
        self.grids = torch.nn.Parameter(eye.view(1, 12, 1, 1, 1).repeat(num, 1, grid_W, grid_Y, grid_X))

    def forward(self, image: torch.Tensor, idx) -> torch.Tensor:
        return slice_image(self.grids, image, idx)

    def tv_loss(self) -> torch.Tensor:
        return total_variation_loss(self.grids)
