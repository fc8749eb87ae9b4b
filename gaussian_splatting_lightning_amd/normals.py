"""Normal consistency (2DGS, Huang et al., SIGGRAPH 2024) on the HIP kernels of csrc/gsr_normals.hip.

The depth distortion map (rasterizer's `distortion=`) thins the surface; this is the other half of the geometry
regularisation of 2DGS, gsplat's 2DGS trainer, PGSR and RaDe-GS, and flattens it: the normals rendered from the
Gaussians must agree with the normals of the rendered depth surface.

* `geometry_features(means3D, scales, rotations, settings_or_viewmatrix)` -> (P,4): per Gaussian the axis of its
  smallest (activated) scale, in view space and facing the camera, and the view depth z -- the feature block to render
  with `features=`.  One launch each way.  Gradients go to `rotations` (through the normal and the quaternion's
  normalisation) and to `means3D` (through z only); the axis choice and the flip are piecewise constant, so `scales`
  gets none.  The camera gets no gradient through the features: a viewmatrix that requires grad is refused with
  NotImplementedError (it still gets its gradient through the rasterizer).
* `normal_consistency(depth, alpha, normals, settings)` -> E (1,H,W) = 1 - stopgrad(alpha) (normals . n_d), n_d the unit
  normals of the surface d = depth / alpha un-projected through the pixel rays (2DGS's depth_to_normal; 0 on the
  one-pixel border and where alpha == 0 all around).  One pass each way; the backward is a gather with no atomics and
  the same bits on every call.  The loss is `lambda * E.mean()`, taken by the caller as with the distortion map.
  With `median_depth=m, depth_ratio=r` the surface is the blend d = (1 - r) depth / alpha + r m of the expected depth
  and the rasterizer's median depth map (`median_depth=True`): r = 1 is 2DGS's setting for bounded scenes, r = 0 its
  setting for unbounded ones.  The backward gives (1 - r) of the surface's gradient to the expected-depth path and r of
  it to `m`, from where it flows into the rasterizer.  Without a median (or with r = 0) the call is bit for bit the
  one above.
* `depth_to_normal(depth, alpha, settings)` -> n_d (3,H,W), no gradient, for visualisation (the same two arguments).
* `render_normal_consistency(rasterizer, ...)` -> (color, radii, invdepth, alpha, E, rendered_normals): the three steps
  in one call for a caller with no feature channels of their own; with `depth_ratio=r` non-zero and a rasterizer built
  with `median_depth=True`, on the blended surface, and `median_depth` is returned as a last element.

`depth` is the rendered sum of w z (feature channel 3), `normals` the rendered feature channels 0-2, un-normalised as
in 2DGS, `alpha` the rasterizer's `return_alpha=True` output.  Pixel (x, y) looks along ((x + 0.5 - W/2) / fx,
(y + 0.5 - H/2) / fy, 1), fx = W / (2 tanfovx): the centred principal point the rasterizer assumes.  Out of scope:
the camera gradient through the features, batched images, non-centred principal points.  Device fp32 contiguous tensors only; no CPU fallback.
"""
from __future__ import annotations

import math

import torch

from . import _native
from .rasterizer import GaussianRasterizationSettings, _stream_handle

__all__ = ["geometry_features", "normal_consistency", "depth_to_normal", "render_normal_consistency",
           "GeometryFeatures", "NormalConsistency", "SurfaceNormalConsistency"]


def _check(what: str, **tensors) -> None:
    for name, t in tensors.items():
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{what}: {name} must be a tensor")
        if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
            raise ValueError(f"{what}: {name} must be a contiguous fp32 device tensor")


def _viewmatrix(settings_or_viewmatrix) -> torch.Tensor:
    vm = settings_or_viewmatrix
    if isinstance(vm, GaussianRasterizationSettings) or hasattr(vm, "viewmatrix"):
        vm = vm.viewmatrix
    if not isinstance(vm, torch.Tensor) or vm.shape != (4, 4):
        raise ValueError("geometry_features: viewmatrix (4,4) expected")
    if vm.requires_grad:
        raise NotImplementedError("geometry_features: no camera gradient through the features; pass "
                                  "viewmatrix.detach() (the rasterizer still gives the camera its gradient)")
    return vm


def _check_gaussians(means3D, scales, rotations, vm) -> int:
    for name, t, w in (("means3D", means3D, 3), ("scales", scales, 3), ("rotations", rotations, 4)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[1] != w:
            raise ValueError(f"geometry_features: {name} (P,{w}) expected")
    P = means3D.shape[0]
    if scales.shape[0] != P or rotations.shape[0] != P:
        raise ValueError("geometry_features: means3D, scales and rotations must have the same number of rows")
    _check("geometry_features", means3D=means3D, scales=scales, rotations=rotations, viewmatrix=vm)
    return P


class GeometryFeatures(torch.autograd.Function):
    """g (P,4) = GeometryFeatures.apply(means3D, scales, rotations, viewmatrix)."""

    @staticmethod
    def forward(ctx, means3D, scales, rotations, viewmatrix):
        P = _check_gaussians(means3D, scales, rotations, viewmatrix)
        out = torch.empty(P, 4, dtype=torch.float32, device=means3D.device)
        if P > 0:
            lib = _native.load()
            _native.check(lib.gsr_geomfeat_forward(P, means3D.data_ptr(), scales.data_ptr(), rotations.data_ptr(),
                                                   viewmatrix.data_ptr(), out.data_ptr(),
                                                   _stream_handle(means3D.device)), "gsr_geomfeat_forward")
        ctx.save_for_backward(means3D, scales, rotations, viewmatrix)
        return out

    @staticmethod
    def backward(ctx, d_out):
        means3D, scales, rotations, viewmatrix = ctx.saved_tensors
        P = means3D.shape[0]
        d_out = d_out.contiguous()
        d_means, d_rot = torch.empty_like(means3D), torch.empty_like(rotations)
        if P > 0:
            lib = _native.load()
            _native.check(lib.gsr_geomfeat_backward(P, means3D.data_ptr(), scales.data_ptr(), rotations.data_ptr(),
                                                    viewmatrix.data_ptr(), d_out.data_ptr(), d_means.data_ptr(),
                                                    d_rot.data_ptr(), _stream_handle(means3D.device)),
                          "gsr_geomfeat_backward")
        return d_means, None, d_rot, None


def geometry_features(means3D: torch.Tensor, scales: torch.Tensor, rotations: torch.Tensor,
                      settings_or_viewmatrix) -> torch.Tensor:
    """(P,4) = (n_v, z) per Gaussian: see the module docstring.  `scales` are the activated scales, `rotations` the
    (w,x,y,z) quaternions, normalised here; the last argument is a GaussianRasterizationSettings or a (4,4) row-vector
    viewmatrix on the device, which must not require grad (NotImplementedError)."""
    return GeometryFeatures.apply(means3D, scales, rotations, _viewmatrix(settings_or_viewmatrix))


def _image_args(what: str, settings, depth, alpha, normals=None):
    H, W = int(settings.image_height), int(settings.image_width)
    tx, ty = float(settings.tanfovx), float(settings.tanfovy)
    if H <= 0 or W <= 0:
        raise ValueError(f"{what}: image_height and image_width must be positive")
    if not (math.isfinite(tx) and math.isfinite(ty) and tx > 0 and ty > 0):
        raise ValueError(f"{what}: tanfovx and tanfovy must be finite and positive")
    named = dict(depth=(depth, 1), alpha=(alpha, 1))
    if normals is not None:
        named["normals"] = (normals, 3)
    for name, (t, c) in named.items():
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != (c, H, W):
            raise ValueError(f"{what}: {name} ({c},{H},{W}) expected from the settings' image_height and image_width")
    _check(what, **{name: t for name, (t, _) in named.items()})
    return H, W, tx, ty


class NormalConsistency(torch.autograd.Function):
    """E (1,H,W) = NormalConsistency.apply(depth, alpha, normals, H, W, tanfovx, tanfovy)."""

    @staticmethod
    def forward(ctx, depth, alpha, normals, H, W, tanfovx, tanfovy):
        E = torch.empty_like(depth)
        lib = _native.load()
        _native.check(lib.gsr_normal_consistency_forward(H, W, tanfovx, tanfovy, depth.data_ptr(), alpha.data_ptr(),
                                                         normals.data_ptr(), E.data_ptr(), None,
                                                         _stream_handle(depth.device)),
                      "gsr_normal_consistency_forward")
        ctx.save_for_backward(depth, alpha, normals)
        ctx.image = (H, W, tanfovx, tanfovy)
        return E

    @staticmethod
    def backward(ctx, d_E):
        depth, alpha, normals = ctx.saved_tensors
        d_E = d_E.contiguous()
        d_depth, d_alpha, d_normals = torch.empty_like(depth), torch.empty_like(alpha), torch.empty_like(normals)
        lib = _native.load()
        _native.check(lib.gsr_normal_consistency_backward(*ctx.image, depth.data_ptr(), alpha.data_ptr(),
                                                          normals.data_ptr(), d_E.data_ptr(), d_depth.data_ptr(),
                                                          d_alpha.data_ptr(), d_normals.data_ptr(),
                                                          _stream_handle(depth.device)),
                      "gsr_normal_consistency_backward")
        return d_depth, d_alpha, d_normals, None, None, None, None


class SurfaceNormalConsistency(torch.autograd.Function):
    """E (1,H,W) = SurfaceNormalConsistency.apply(depth, alpha, normals, median_depth, depth_ratio, H, W, tanfovx,
    tanfovy): NormalConsistency on the surface (1 - depth_ratio) depth / alpha + depth_ratio median_depth."""

    @staticmethod
    def forward(ctx, depth, alpha, normals, median, ratio, H, W, tanfovx, tanfovy):
        E = torch.empty_like(depth)
        lib = _native.load()
        _native.check(lib.gsr_normal_consistency_forward_surface(
            H, W, tanfovx, tanfovy, depth.data_ptr(), alpha.data_ptr(), normals.data_ptr(), median.data_ptr(), ratio,
            E.data_ptr(), None, _stream_handle(depth.device)), "gsr_normal_consistency_forward_surface")
        ctx.save_for_backward(depth, alpha, normals, median)
        ctx.image = (H, W, tanfovx, tanfovy)
        ctx.ratio = ratio
        return E

    @staticmethod
    def backward(ctx, d_E):
        depth, alpha, normals, median = ctx.saved_tensors
        d_E = d_E.contiguous()
        d_depth, d_alpha, d_normals = torch.empty_like(depth), torch.empty_like(alpha), torch.empty_like(normals)
        d_median = torch.empty_like(median)
        lib = _native.load()
        _native.check(lib.gsr_normal_consistency_backward_surface(
            *ctx.image, depth.data_ptr(), alpha.data_ptr(), normals.data_ptr(), median.data_ptr(), ctx.ratio,
            d_E.data_ptr(), d_depth.data_ptr(), d_alpha.data_ptr(), d_normals.data_ptr(), d_median.data_ptr(),
            _stream_handle(depth.device)), "gsr_normal_consistency_backward_surface")
        return d_depth, d_alpha, d_normals, d_median, None, None, None, None, None


def _surface_args(what: str, settings, median_depth, depth_ratio):
    """The depth ratio as a float and whether the blended surface is asked for: a median map and a non-zero ratio (a
    zero ratio, or no median, is the expected-depth surface: the call it always was).  ValueError for a ratio that is
    not finite, for a non-zero ratio without a median, and for a median that is not a (1,H,W) fp32 device tensor."""
    r = float(depth_ratio)
    if not math.isfinite(r):
        raise ValueError(f"{what}: depth_ratio must be finite")
    if median_depth is None:
        if r != 0.0:
            raise ValueError(f"{what}: depth_ratio={r} needs median_depth (the rasterizer's median_depth=True output)")
        return r, False
    H, W = int(settings.image_height), int(settings.image_width)
    if not isinstance(median_depth, torch.Tensor) or tuple(median_depth.shape) != (1, H, W):
        raise ValueError(f"{what}: median_depth (1,{H},{W}) expected from the settings' image_height and image_width")
    _check(what, median_depth=median_depth)
    return r, r != 0.0


def normal_consistency(depth: torch.Tensor, alpha: torch.Tensor, normals: torch.Tensor, settings,
                       median_depth=None, depth_ratio: float = 0.0) -> torch.Tensor:
    """E (1,H,W) = 1 - stopgrad(alpha) (normals . n_d): see the module docstring.  `settings` is a
    GaussianRasterizationSettings; tanfovx, tanfovy, image_height and image_width are read.  median_depth (1,H,W) and
    depth_ratio r: n_d is taken from the surface (1 - r) depth / alpha + r median_depth, and median_depth receives r of
    the surface's gradient; with median_depth=None or r = 0 the call is bitwise the one without them."""
    H, W, tx, ty = _image_args("normal_consistency", settings, depth, alpha, normals)
    r, blend = _surface_args("normal_consistency", settings, median_depth, depth_ratio)
    if not blend:
        return NormalConsistency.apply(depth, alpha, normals, H, W, tx, ty)
    return SurfaceNormalConsistency.apply(depth, alpha, normals, median_depth, r, H, W, tx, ty)


@torch.no_grad()
def depth_to_normal(depth: torch.Tensor, alpha: torch.Tensor, settings, median_depth=None,
                    depth_ratio: float = 0.0) -> torch.Tensor:
    """n_d (3,H,W), the depth normals `normal_consistency` compares with (the same bits, of the same surface), without
    a gradient."""
    H, W, tx, ty = _image_args("depth_to_normal", settings, depth, alpha)
    r, blend = _surface_args("depth_to_normal", settings, median_depth, depth_ratio)
    n_d = torch.empty(3, H, W, dtype=torch.float32, device=depth.device)
    lib = _native.load()
    if blend:
        _native.check(lib.gsr_depth_to_normal_surface(H, W, tx, ty, depth.data_ptr(), alpha.data_ptr(),
                                                      median_depth.data_ptr(), r, n_d.data_ptr(),
                                                      _stream_handle(depth.device)), "gsr_depth_to_normal_surface")
        return n_d
    _native.check(lib.gsr_depth_to_normal(H, W, tx, ty, depth.data_ptr(), alpha.data_ptr(), n_d.data_ptr(),
                                          _stream_handle(depth.device)), "gsr_depth_to_normal")
    return n_d


def render_normal_consistency(rasterizer, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None,
                              rotations=None, depth_ratio: float = 0.0):
    """(color, radii, invdepth, alpha, E, rendered_normals) of one view.  `rasterizer` is a GaussianRasterizer built
    with return_alpha=True (and no distortion map); `scales` and `rotations` are the activated ones it renders with.
    A thin convenience with no kernel of its own: geometry_features, the rasterizer with features= that block, then
    normal_consistency(F[3:4], alpha, F[0:3], settings).  A caller who also renders feature channels of their own
    appends them to the block and uses the three pieces directly.
    depth_ratio non-zero: `rasterizer` must also be built with median_depth=True; E is then taken on the surface
    (1 - depth_ratio) depth / alpha + depth_ratio median_depth.  A rasterizer built with median_depth=True makes the
    call return median_depth (1,H,W) as a last, seventh element, whatever the ratio."""
    r = float(depth_ratio)
    if not math.isfinite(r):
        raise ValueError("render_normal_consistency: depth_ratio must be finite")
    with_median = bool(getattr(rasterizer, "median_depth", False))
    if r != 0.0 and not with_median:
        raise ValueError("render_normal_consistency: a non-zero depth_ratio needs a GaussianRasterizer(settings, "
                         "return_alpha=True, median_depth=True)")
    if not getattr(rasterizer, "return_alpha", False) or getattr(rasterizer, "distortion", None) is not None:
        raise ValueError("render_normal_consistency: a GaussianRasterizer(settings, return_alpha=True) without a "
                         "distortion map expected")
    if scales is None or rotations is None:
        raise ValueError("render_normal_consistency: scales and rotations expected (the normals come from them)")
    rs = rasterizer.raster_settings
    g = geometry_features(means3D, scales, rotations, rs.viewmatrix.detach())
    out = rasterizer(means3D=means3D, means2D=means2D, opacities=opacities, shs=shs, colors_precomp=colors_precomp,
                     scales=scales, rotations=rotations, features=g)
    color, radii, invdepth, alpha, F = out[:5]
    normals = F[0:3].contiguous()
    if not with_median:
        E = normal_consistency(F[3:4].contiguous(), alpha, normals, rs)
        return color, radii, invdepth, alpha, E, normals
    E = normal_consistency(F[3:4].contiguous(), alpha, normals, rs, median_depth=out[5], depth_ratio=r)
    return color, radii, invdepth, alpha, E, normals, out[5]
