"""The 3D smoothing filter of Mip-Splatting (Yu et al., CVPR 2024) on the HIP kernels of csrc/gsr_mipfilter.hip.

The rasterizer's `antialiasing=True` is the paper's 2D screen-space filter; this is its other half.  Every Gaussian is
bounded from below by the finest sampling any training camera has of it: with nu_i = max_k fx_k / z_ik over the cameras
that see it, `filter_3D_i = sqrt(0.2) / nu_i`, and the activations that feed the rasterizer become

    s' = sqrt(s^2 + filter_3D^2),   o' = o * prod_k (s_k / s'_k)

(the Gaussian convolved with an isotropic one of that size, its integral o prod s kept).  The compensation is formed as
the product of the three ratios: the published sqrt(prod s^2 / prod s'^2) underflows in fp32 from raw scalings near -15.

* `sampling_rate(means3D, cameras)`      -- (rate, zmin, seen) over all cameras in one launch (gsr_mipfilter_rate)
* `compute_3d_filter(means3D, cameras)`  -- filter_3D (P,1); a handful of torch ops on those, no host synchronisation
* `activate_filtered` / `activate_filtered_backward` / `FilteredGaussianActivations` -- one launch each way, the
  counterpart of activations.py; rows with filter_3D == 0 are `activate`'s bit for bit

A camera sees a Gaussian when z > near, |x| <= (1 + 2 margin) tanfovx z and |y| <= (1 + 2 margin) tanfovy z in its view
space (p_view = [p, 1] viewmatrix): the rasterizer's near plane, and Mip-Splatting's 15 % border around the image.
`cameras` is a sequence of GaussianRasterizationSettings (viewmatrix, tanfovx, tanfovy, image_width, image_height are
read) or a dict of stacked tensors viewmatrix (V,4,4), tanfovx (V), tanfovy (V), width (V), height (V).  Recompute the
filter whenever the set of Gaussians changes (upstream: every 100 steps and after each densification).
Device fp32 tensors only; no CPU fallback.
"""
from __future__ import annotations

import math
from typing import Tuple

import torch

from . import _native
from .rasterizer import _stream_handle

__all__ = ["sampling_rate", "compute_3d_filter", "camera_table", "activate_filtered", "activate_filtered_backward",
           "FilteredGaussianActivations", "MODES"]

MODES = ("per_camera", "shared_focal")
_CAMERA_KEYS = ("viewmatrix", "tanfovx", "tanfovy", "width", "height")


def _stacked(cameras) -> dict:
    """The cameras as float64 tensors viewmatrix (V,4,4), tanfovx, tanfovy, width, height (V), wherever they live."""
    if isinstance(cameras, dict):
        missing = [k for k in _CAMERA_KEYS if k not in cameras]
        if missing:
            raise ValueError(f"mipfilter: cameras lacks {missing}")
        c = {k: torch.as_tensor(cameras[k]) for k in _CAMERA_KEYS}
    else:
        cams = list(cameras)
        if not cams:
            raise ValueError("mipfilter: cameras is empty, at least one camera expected")
        c = dict(viewmatrix=torch.stack([torch.as_tensor(s.viewmatrix) for s in cams]),
                 tanfovx=torch.tensor([float(s.tanfovx) for s in cams], dtype=torch.float64),
                 tanfovy=torch.tensor([float(s.tanfovy) for s in cams], dtype=torch.float64),
                 width=torch.tensor([float(s.image_width) for s in cams], dtype=torch.float64),
                 height=torch.tensor([float(s.image_height) for s in cams], dtype=torch.float64))
    V = c["viewmatrix"].shape[0] if c["viewmatrix"].dim() else 0
    if V == 0:
        raise ValueError("mipfilter: cameras is empty, at least one camera expected")
    if c["viewmatrix"].shape != (V, 4, 4) or any(c[k].shape != (V,) for k in _CAMERA_KEYS[1:]):
        raise ValueError("mipfilter: expected viewmatrix (V,4,4) and tanfovx, tanfovy, width, height (V)")
    return c


def camera_table(cameras, margin: float = 0.15, device="cuda") -> Tuple[torch.Tensor, torch.Tensor]:
    """(table (V,16) fp32, fx (V) fp32) on `device`: row k = [viewmatrix[:,2] | viewmatrix[:,0] | viewmatrix[:,1] |
    fx, (1 + 2 margin) tanfovx, (1 + 2 margin) tanfovy, 0], the layout gsr_mipfilter_rate reads.
    fx and the limits are formed in float64 and rounded once."""
    c = {k: v.to(device=device, dtype=torch.float64) for k, v in _stacked(cameras).items()}
    vm = c["viewmatrix"]
    fx = c["width"] / (2.0 * c["tanfovx"])
    band = 1.0 + 2.0 * float(margin)
    zero = torch.zeros_like(fx)
    table = torch.cat([vm[:, :, 2], vm[:, :, 0], vm[:, :, 1],
                       torch.stack([fx, band * c["tanfovx"], band * c["tanfovy"], zero], 1)], 1)
    return table.to(torch.float32).contiguous(), fx.to(torch.float32)


def _check_means(means3D: torch.Tensor) -> None:
    if not isinstance(means3D, torch.Tensor) or means3D.dim() != 2 or means3D.shape[1] != 3:
        raise ValueError("mipfilter: means3D (P,3) expected")
    if means3D.dtype != torch.float32 or not means3D.is_cuda or not means3D.is_contiguous():
        raise ValueError("mipfilter: means3D must be a contiguous fp32 device tensor")


def _rates(means3D, cameras, near, margin):
    if not math.isfinite(near) or not math.isfinite(margin) or margin < 0:
        raise ValueError("mipfilter: near must be finite and margin finite and non-negative")
    stacked = _stacked(cameras)  # refusals before the device is asked for anything
    _check_means(means3D)
    P, dev = means3D.shape[0], means3D.device
    table, fx = camera_table(stacked, margin, dev)
    rate = torch.empty(P, dtype=torch.float32, device=dev)
    zmin = torch.empty(P, dtype=torch.float32, device=dev)
    seen = torch.empty(P, dtype=torch.int32, device=dev)
    if P > 0:
        lib = _native.load()
        _native.check(lib.gsr_mipfilter_rate(P, means3D.data_ptr(), table.shape[0], table.data_ptr(), float(near),
                                             rate.data_ptr(), zmin.data_ptr(), seen.data_ptr(), _stream_handle(dev)),
                      "gsr_mipfilter_rate")
    return rate, zmin, seen, fx


@torch.no_grad()
def sampling_rate(means3D: torch.Tensor, cameras, near: float = 0.2, margin: float = 0.15):
    """(rate (P,), zmin (P,), seen (P,) int32): over the cameras that see Gaussian i, the maximum of fx_k / z_ik (the
    paper's maximal sampling rate; 0 where none sees it), the minimum depth (+inf where none), and their number."""
    return _rates(means3D, cameras, near, margin)[:3]


@torch.no_grad()
def compute_3d_filter(means3D: torch.Tensor, cameras, variance: float = 0.2, mode: str = "per_camera",
                      near: float = 0.2, margin: float = 0.15) -> torch.Tensor:
    """filter_3D (P,1).  mode "per_camera": sqrt(variance) / rate_i; "shared_focal": sqrt(variance) zmin_i / max_k fx_k,
    the released Mip-Splatting code's form (the same when all focals are equal).  A Gaussian no camera sees gets the
    largest value among the seen ones; when none is seen at all the filter is 0 (the identity)."""
    if mode not in MODES:
        raise ValueError(f"mipfilter: mode must be one of {MODES}, got {mode!r}")
    if not (variance >= 0 and math.isfinite(variance)):
        raise ValueError("mipfilter: variance must be finite and non-negative")
    rate, zmin, seen, fx = _rates(means3D, cameras, near, margin)
    if means3D.shape[0] == 0:
        return rate[:, None]
    sd = math.sqrt(variance)
    f = sd / rate if mode == "per_camera" else sd * zmin / fx.max()
    vis = seen > 0
    f = torch.where(vis, f, torch.zeros_like(f))
    return torch.where(vis, f, f.max())[:, None].contiguous()


def _check(*ts: torch.Tensor) -> None:
    for t in ts:
        if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("filtered activations: contiguous fp32 device tensors expected")


def activate_filtered(scaling: torch.Tensor, opacity: torch.Tensor, rotation: torch.Tensor, filter_3D: torch.Tensor,
                      out=None):
    """(sqrt(exp(scaling)^2 + filter_3D^2), sigmoid(opacity) prod_k s_k / s'_k, normalize(rotation)); out = optional
    preallocated (scales, opacities, rotations).  filter_3D (N) or (N,1), non-negative."""
    N = scaling.shape[0]
    if (scaling.shape != (N, 3) or opacity.numel() != N or rotation.shape != (N, 4) or filter_3D.numel() != N
            or filter_3D.dim() not in (1, 2)):
        raise ValueError("filtered activations: expected scaling (N,3), opacity (N) or (N,1), rotation (N,4), "
                         "filter_3D (N) or (N,1)")
    if out is None:
        out = (torch.empty_like(scaling), torch.empty_like(opacity), torch.empty_like(rotation))
    if tuple(o.numel() for o in out) != (3 * N, N, 4 * N):
        raise ValueError("filtered activations: out must hold (N,3), (N) and (N,4) elements")
    _check(scaling, opacity, rotation, filter_3D, *out)
    if N > 0:
        lib = _native.load()
        _native.check(lib.gsr_activations_filter3d_forward(
            N, scaling.data_ptr(), opacity.data_ptr(), rotation.data_ptr(), filter_3D.data_ptr(), out[0].data_ptr(),
            out[1].data_ptr(), out[2].data_ptr(), _stream_handle(scaling.device)), "gsr_activations_filter3d_forward")
    return out


def activate_filtered_backward(scaling: torch.Tensor, opacity: torch.Tensor, rotation: torch.Tensor,
                               filter_3D: torch.Tensor, dL_dscales: torch.Tensor, dL_dopacities: torch.Tensor,
                               dL_drotations: torch.Tensor, out=None):
    """Gradients w.r.t. the raw (scaling, opacity, rotation) from those w.r.t. the filtered activations.  Takes the
    forward's inputs, not its outputs: the kernel recomputes s, s' and o from them.  filter_3D takes no gradient."""
    N = scaling.shape[0]
    if scaling.shape != (N, 3) or opacity.numel() != N or rotation.shape != (N, 4) or filter_3D.numel() != N:
        raise ValueError("filtered activations: expected scaling (N,3), opacity (N) or (N,1), rotation (N,4), "
                         "filter_3D (N) or (N,1)")
    for t, w in ((dL_dscales, 3), (dL_dopacities, 1), (dL_drotations, 4)):
        if t.numel() != N * w:
            raise ValueError("filtered activations: gradient shapes do not match N")
    if out is None:
        out = (torch.empty_like(scaling), torch.empty_like(opacity), torch.empty_like(rotation))
    if tuple(o.numel() for o in out) != (3 * N, N, 4 * N):
        raise ValueError("filtered activations: out must hold (N,3), (N) and (N,4) elements")
    _check(scaling, opacity, rotation, filter_3D, dL_dscales, dL_dopacities, dL_drotations, *out)
    if N > 0:
        lib = _native.load()
        _native.check(lib.gsr_activations_filter3d_backward(
            N, scaling.data_ptr(), opacity.data_ptr(), rotation.data_ptr(), filter_3D.data_ptr(),
            dL_dscales.data_ptr(), dL_dopacities.data_ptr(), dL_drotations.data_ptr(), out[0].data_ptr(),
            out[1].data_ptr(), out[2].data_ptr(), _stream_handle(scaling.device)), "gsr_activations_filter3d_backward")
    return out


class FilteredGaussianActivations(torch.autograd.Function):
    """scales, opacities, rotations = FilteredGaussianActivations.apply(_scaling, _opacity, _rotation, filter_3D)."""

    @staticmethod
    def forward(ctx, scaling, opacity, rotation, filter_3D):
        scaling, opacity, rotation = scaling.contiguous(), opacity.contiguous(), rotation.contiguous()
        filter_3D = filter_3D.detach().contiguous()
        out = activate_filtered(scaling, opacity, rotation, filter_3D)
        ctx.save_for_backward(scaling, opacity, rotation, filter_3D)
        return out

    @staticmethod
    def backward(ctx, d_scales, d_opacities, d_rotations):
        scaling, opacity, rotation, filter_3D = ctx.saved_tensors
        z = torch.zeros_like
        d_scales = z(scaling) if d_scales is None else d_scales.contiguous()
        d_opacities = z(opacity) if d_opacities is None else d_opacities.contiguous()
        d_rotations = z(rotation) if d_rotations is None else d_rotations.contiguous()
        return (*activate_filtered_backward(scaling, opacity, rotation, filter_3D, d_scales, d_opacities, d_rotations),
                None)
