"""Host-side mirror of the `diff_gaussian_rasterization` Python API, backed by libgsrast.so.

The reference calls this API at
    gs_lightning/lightning/gs_lightning_module.py:322-348   (training: settings, rasterizer(...), means2D grad)
    scripts/render_trained_image.py:98-124                  (inference: means2D=None)
    tests/rasterizer_python/test_mark_visible.py:13-14       (GaussianRasterizer(s).markVisible(points))
The names, argument meaning, return values and error behaviour are those of the upstream package
(graphdeco-inria/diff-gaussian-rasterization@dr_aa):
    GaussianRasterizationSettings   13-field NamedTuple
    GaussianRasterizer(settings)(means3D, means2D, opacities, shs, colors_precomp, scales, rotations,
                                 cov3D_precomp) -> (color (3,H,W), radii (P,) int32, invdepth (1,H,W))
    GaussianRasterizer.markVisible(positions) -> bool (P,)
    rasterize_gaussians(...)        functional form
Beyond upstream: GaussianRasterizer(settings, return_alpha=True) / rasterize_gaussians(..., return_alpha=True) also
return alpha (1,H,W) = 1 - final transmittance, and settings.bg may be a (3,H,W) image and receives a gradient where
it requires grad (gsr_forward_ext / gsr_backward_ext); without either the call is upstream's.
GaussianRasterizer(settings, absgrad=True) / rasterize_gaussians(..., absgrad=True) set means2D.absgrad (P,3) in the
backward, as gsplat does: the absolute screen-space gradient of AbsGS for densification (gsr_backward_abs).
rasterizer(..., features=f) / rasterize_gaussians(..., features=f) with f (P,C), 1 <= C <= 64, also return the feature
image (C,H,W) = sum_i alpha_i T_i f[i] (no background) as the last output, differentiable with respect to f and,
through alpha, to everything the colour is (gsr_forward_features / gsr_backward_features).
GaussianRasterizer(settings, distortion="z" | "ndc") / rasterize_gaussians(..., distortion=...) also return the depth
distortion map (1,H,W) = sum_i sum_j w_i w_j |t_i - t_j| of Mip-NeRF 360 (2DGS's distloss) as the last output, after
the feature image: t the view depth ("z") or 2DGS's far / (far - near) (1 - near / z) ("ndc", distortion_near /
distortion_far), differentiable through the weights and through t (gsr_forward_distortion / gsr_backward_distortion).
GaussianRasterizer(settings, median_depth=True) / rasterize_gaussians(..., median_depth=True) also return, as the last two
outputs, median_depth (1,H,W) float32 and median_index (1,H,W) int32: the view depth and the id of the Gaussian at which
the pixel's transmittance crosses 1/2 (2DGS's depth_ratio = 1 surface; 0 and -1 where no Gaussian reaches).  The depth
is differentiable with respect to the selected Gaussian's depth alone (gsr_forward_median / gsr_backward_median).
Every computation runs in the HIP kernels on the tensors' device; the scratch state the backward needs
(geometry/binning/image buffers) lives in uint8 tensors saved on the autograd context.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional

import torch
import torch.nn as nn

from . import _native


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool
    antialiasing: bool


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    if t is None or t.numel() == 0:
        return None
    return t.data_ptr()


def _prep(t: Optional[torch.Tensor], device, name: str) -> Optional[torch.Tensor]:
    if t is None or t.numel() == 0:
        return None
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name} must be float32 (got {t.dtype})")
    if t.device != device:
        t = t.to(device)
    return t.contiguous()


class _Buffers:
    """Caller-owned scratch buffers grown through the C callback (reference: resizeFunctional).

    The callback is a closure over the buffer dict, not a bound method: a bound method would make a reference
    cycle (object -> callback -> method -> object), so the buffers (GBs at 5M Gaussians / 4K) would outlive the
    call until the cyclic garbage collector ran -- never, while it is disabled (bench.py's timed region),
    which ran the device out of memory.  An exception inside the callback (e.g. torch.OutOfMemoryError) is
    kept and re-raised after the library call; the callback then returns NULL, which the library reports as
    GSR_ERR_ALLOC (a ctypes callback that raises would hand the library an undefined pointer)."""

    def __init__(self, device):
        self.device = device
        self.bufs = bufs = {}
        self.errors = errors = []

        def alloc(_ctx, which, nbytes):
            try:
                t = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)
            except BaseException as e:  # noqa: BLE001 -- re-raised by raise_pending()
                errors.append(e)
                return None
            bufs[int(which)] = t
            return t.data_ptr()

        self._cb = _native.ALLOC_FN(alloc)

    @property
    def callback(self):
        return self._cb

    def raise_pending(self):
        if self.errors:
            raise self.errors[0]

    def get(self, which) -> torch.Tensor:
        t = self.bufs.get(which)
        return t if t is not None else torch.empty(0, dtype=torch.uint8, device=self.device)


def _stream_handle(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


class ForwardState(NamedTuple):
    """Everything the backward needs from one forward call (tensors kept alive by autograd)."""
    means3D: torch.Tensor
    shs: Optional[torch.Tensor]
    colors_precomp: Optional[torch.Tensor]
    opacities: torch.Tensor
    scales: Optional[torch.Tensor]
    rotations: Optional[torch.Tensor]
    cov3D_precomp: Optional[torch.Tensor]
    radii: torch.Tensor
    bg: torch.Tensor
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    campos: Optional[torch.Tensor]
    geom_buffer: torch.Tensor
    binning_buffer: torch.Tensor
    image_buffer: torch.Tensor
    num_rendered: int
    num_big: int
    M: int
    features: Optional[torch.Tensor] = None  # the prepared (P,C) feature channels, when the forward was given any


class DistortionState(NamedTuple):
    """What a forward with a distortion map leaves for its backward: the map and its planes, and the per-pixel totals
    (2,H,W) = (sum_i w_i, sum_i w_i t_i) the reverse walk takes its prefix sums from."""
    map: str
    near: float
    far: float
    totals: torch.Tensor


class MedianState(NamedTuple):
    """What a forward with a median depth map leaves for its backward: per pixel the selected pair's position in its
    tile's sorted list, (H,W) int32, -1 where no Gaussian reaches."""
    pos: torch.Tensor


class _ExtendedForwardState(ForwardState):
    """A ForwardState that also carries a DistortionState as .distortion and / or a MedianState as .median --
    attributes, not fields: the fields of ForwardState, their count and their order are what earlier callers construct
    and index."""
    distortion: Optional[DistortionState] = None
    median: Optional[MedianState] = None


_DistortionForwardState = _ExtendedForwardState  # its name while the distortion map was the only such attribute


def _distortion(distortion, near, far):
    """(map name, near, far) of a distortion request, or None for None; RuntimeError for an unknown map, and for planes
    that are not 0 < near < far ("ndc" needs both; "z" reads neither, but refuses bad ones)."""
    if distortion is None:
        return None
    if distortion not in _native.DISTORTION_MAPS:
        raise RuntimeError(f"distortion must be one of {sorted(_native.DISTORTION_MAPS)} or None, got {distortion!r}")
    if distortion == "ndc" and (near is None or far is None):
        raise RuntimeError("distortion='ndc' needs distortion_near and distortion_far")
    near = 0.0 if near is None else float(near)
    far = 0.0 if far is None else float(far)
    if (distortion == "ndc" or near or far) and not (0.0 < near < far < float("inf")):
        raise RuntimeError(f"distortion needs 0 < distortion_near < distortion_far, got near={near}, far={far}")
    return distortion, near, far


def _background(bg, H: int, W: int) -> bool:
    """Whether a background tensor is a per-pixel (3,H,W) image (True) or the (3,) vector; RuntimeError otherwise."""
    if bg is not None and tuple(bg.shape) == (3,):
        return False
    if bg is not None and tuple(bg.shape) == (3, H, W):
        return True
    raise RuntimeError(f"bg must have shape (3,) or (3, {H}, {W}), got {None if bg is None else tuple(bg.shape)}")


def _features(features, P: int, device):
    """The feature channels as a contiguous float32 (P,C) tensor on the device, 1 <= C <= 64; RuntimeError otherwise."""
    if not torch.is_tensor(features) or features.ndim != 2 or features.shape[0] != P:
        raise RuntimeError(f"features must have shape ({P}, C), got "
                           f"{tuple(features.shape) if torch.is_tensor(features) else type(features).__name__}")
    C = int(features.shape[1])
    if not 1 <= C <= _native.FEATURES_MAX_C:
        raise RuntimeError(f"features must have between 1 and {_native.FEATURES_MAX_C} channels, got {C}")
    if features.dtype != torch.float32:
        raise RuntimeError(f"features must be float32 (got {features.dtype})")
    if features.device != device:
        features = features.to(device)
    return features.contiguous()


def forward_raw(means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings,
                return_alpha=False, features=None, distortion=None, distortion_near=None, distortion_far=None,
                median_depth=False):
    """One call of gsr_forward.  Returns (color (3,H,W), radii (P,), invdepth (1,H,W), ForwardState).
    raster_settings.bg is the (3,) background or a (3,H,W) image, one background per pixel.  return_alpha=True returns
    (color, radii, invdepth, alpha (1,H,W), ForwardState), alpha = 1 - the transmittance left behind the pixel's last
    contributor (0 where no Gaussian reaches).  Either goes through gsr_forward_ext; the plain call is gsr_forward.
    With P == 0 the two differ in colour: the plain call returns zeros (upstream's early return), the ext call what the
    composite writes where no Gaussian reaches, the background; every P > 0 colour is bitwise the same in both.
    features (P,C), 1 <= C <= 64: the feature image (C,H,W) = sum_i alpha_i T_i features[i], with the colour's weights
    and no background, is returned after alpha and before the state, which keeps the prepared features for the
    backward (gsr_forward_features).  Colour, radii, invdepth and alpha are bitwise those of the call without.
    distortion "z" or "ndc": the depth distortion map (1,H,W) = sum_i sum_j w_i w_j |t_i - t_j| over each pixel's
    contributors, with the colour's weights and no background term (exactly 0 where no Gaussian reaches), is returned
    last before the state, after the feature image; t is the view depth ("z") or far / (far - near) (1 - near / z)
    ("ndc": distortion_near, distortion_far, 0 < near < far).  The state then carries .distortion, a DistortionState
    (gsr_forward_distortion); every other output keeps its bits.
    median_depth=True: median_depth (1,H,W) float32 and median_index (1,H,W) int32 are returned last before the state,
    after the distortion map: the view depth and the id of the last contributor the pixel's transmittance reaches above
    1/2 (the last contributor at all on a pixel that never becomes half opaque; 0 and -1 where no Gaussian reaches).
    The state then carries .median, a MedianState (gsr_forward_median); every other output keeps its bits."""
    dist_spec = _distortion(distortion, distortion_near, distortion_far)
    lib = _native.load()
    device = means3D.device
    if device.type != "cuda":
        raise RuntimeError("the MI355X rasterizer needs its inputs on a HIP device (tensor.device.type == 'cuda')")
    if means3D.ndim != 2 or means3D.shape[1] != 3:
        raise RuntimeError("means3D must have dimensions (num_points, 3)")
    rs = raster_settings
    P = means3D.shape[0]
    H, W = int(rs.image_height), int(rs.image_width)
    means3D_c = _prep(means3D, device, "means3D")
    sh_c = _prep(sh, device, "shs")
    col_c = _prep(colors_precomp, device, "colors_precomp")
    op_c = _prep(opacities, device, "opacities")
    sc_c = _prep(scales, device, "scales")
    rot_c = _prep(rotations, device, "rotations")
    cov_c = _prep(cov3Ds_precomp, device, "cov3D_precomp")
    bg = _prep(rs.bg, device, "bg")
    bg_image = _background(bg, H, W)
    view = _prep(rs.viewmatrix, device, "viewmatrix")
    proj = _prep(rs.projmatrix, device, "projmatrix")
    campos = _prep(rs.campos, device, "campos")
    M = 0 if sh_c is None else (sh_c.shape[1] if sh_c.ndim == 3 else sh_c.shape[1] // 3)
    feat_c = None if features is None else _features(features, P, device)

    # fully written by the library (render_fwd writes every pixel, preprocess every radius; P == 0 clears)
    color = torch.empty(3, H, W, dtype=torch.float32, device=device)
    invdepth = torch.empty(1, H, W, dtype=torch.float32, device=device)
    radii = torch.empty(P, dtype=torch.int32, device=device)
    alpha = torch.empty(1, H, W, dtype=torch.float32, device=device) if return_alpha else None
    ext = None
    if bg_image or return_alpha:
        ext = _native.CompositeExt(background_image=_ptr(bg) if bg_image else None, out_alpha=_ptr(alpha))
    feat_image = feat = None
    if feat_c is not None:
        feat_image = torch.empty(feat_c.shape[1], H, W, dtype=torch.float32, device=device)
        feat = _native.FeaturesExt(C=int(feat_c.shape[1]), features=_ptr(feat_c), out_features=feat_image.data_ptr())
    dist_image = dist = totals = None
    if dist_spec is not None:
        dist_image = torch.empty(1, H, W, dtype=torch.float32, device=device)
        totals = torch.empty(2, H, W, dtype=torch.float32, device=device)
        dist = _native.DistortionExt(map=_native.DISTORTION_MAPS[dist_spec[0]], near_plane=dist_spec[1],
                                     far_plane=dist_spec[2], out_distortion=dist_image.data_ptr(),
                                     total_weight=totals[0].data_ptr(), total_moment=totals[1].data_ptr())
    med_depth = med_index = med_pos = med = None
    if median_depth:
        med_depth = torch.empty(1, H, W, dtype=torch.float32, device=device)
        med_index = torch.empty(1, H, W, dtype=torch.int32, device=device)
        med_pos = torch.empty(H, W, dtype=torch.int32, device=device)
        med = _native.MedianExt(out_median_depth=med_depth.data_ptr(), out_median_index=med_index.data_ptr(),
                                median_pos=med_pos.data_ptr())
    bufs = _Buffers(device)
    a = _native.ForwardArgs(
        P=P, D=int(rs.sh_degree), M=M, W=W, H=H, background=None if bg_image else _ptr(bg), means3D=_ptr(means3D_c),
        colors_precomp=_ptr(col_c), opacities=_ptr(op_c), scales=_ptr(sc_c),
        scale_modifier=float(rs.scale_modifier), rotations=_ptr(rot_c), cov3D_precomp=_ptr(cov_c),
        viewmatrix=_ptr(view), projmatrix=_ptr(proj), campos=_ptr(campos), tan_fovx=float(rs.tanfovx),
        tan_fovy=float(rs.tanfovy), shs=_ptr(sh_c), prefiltered=int(bool(rs.prefiltered)),
        antialiasing=int(bool(rs.antialiasing)), debug=int(bool(rs.debug)), out_color=color.data_ptr(),
        out_invdepth=invdepth.data_ptr(), radii=radii.data_ptr())
    num_rendered = ctypes.c_int64(0)
    with torch.cuda.device(device):  # the library also switches to its stream's device (gsr_api.hip)
        rc = _native.call_forward(lib, a, ext, feat, bufs.callback, _stream_handle(device), num_rendered, dist=dist,
                                  median=med)
    bufs.raise_pending()
    _native.check(rc, "rasterize_gaussians")
    state = ForwardState(means3D_c, sh_c, col_c, op_c, sc_c, rot_c, cov_c, radii, bg, view, proj, campos,
                         bufs.get(_native.GSR_BUF_GEOM), bufs.get(_native.GSR_BUF_BINNING),
                         bufs.get(_native.GSR_BUF_IMAGE), int(num_rendered.value), int(a.num_big_out), M, feat_c)
    res = (color, radii, invdepth) + ((alpha,) if return_alpha else ()) + ((feat_image,) if feat is not None else ())
    if dist is not None or med is not None:
        state = _ExtendedForwardState(*state)
    if dist is not None:
        state.distortion = DistortionState(*dist_spec, totals)
        res += (dist_image,)
    if med is not None:
        state.median = MedianState(med_pos)
        res += (med_depth, med_index)
    return (*res, state)


class _Upstream(NamedTuple):
    """One backward's upstream gradients, contiguous float32 (None where absent), and what follows from them."""
    color: torch.Tensor
    depth: Optional[torch.Tensor]
    alpha: Optional[torch.Tensor]
    features: Optional[torch.Tensor]
    distortion: Optional[torch.Tensor]
    median: Optional[torch.Tensor]
    bg_image: bool                         # the forward's background is a (3,H,W) image
    ext: Optional[_native.CompositeExt]    # the backward's gsr_composite_ext, None for the plain call


def _upstream(st: ForwardState, rs, grad_color, grad_depth, grad_alpha=None, grad_features=None, dbg=None,
              grad_distortion=None, grad_median=None):
    """The upstream gradients of colour (zeros when None), inverse depth, alpha ((1,H,W) or (H,W)) and the feature image
    ((C,H,W), only for a state with features), the distortion map ((1,H,W) or (H,W), only for a state with
    distortion) and the median depth ((1,H,W) or (H,W), only for a state with the median), checked and made contiguous float32, and the call's CompositeExt: given
    with a background image, an alpha gradient or dbg, the destination of the background's gradient."""
    H, W = int(rs.image_height), int(rs.image_width)
    if grad_color is None:
        grad_color = torch.zeros(3, H, W, dtype=torch.float32, device=st.radii.device)
    grad_color = grad_color.to(torch.float32).contiguous()
    if grad_depth is not None:
        grad_depth = grad_depth.to(torch.float32).contiguous()
    if grad_alpha is not None:
        if grad_alpha.numel() != H * W:
            raise RuntimeError(f"grad_out_alpha must have shape (1, {H}, {W}), got {tuple(grad_alpha.shape)}")
        grad_alpha = grad_alpha.to(torch.float32).contiguous()
    if grad_features is not None:
        if st.features is None:
            raise RuntimeError("grad_out_features needs a state from forward_raw(..., features=...)")
        C = int(st.features.shape[1])
        if tuple(grad_features.shape) != (C, H, W):
            raise RuntimeError(f"grad_out_features must have shape ({C}, {H}, {W}), got {tuple(grad_features.shape)}")
        grad_features = grad_features.to(torch.float32).contiguous()
    if grad_distortion is not None:
        if getattr(st, "distortion", None) is None:
            raise RuntimeError("grad_out_distortion needs a state from forward_raw(..., distortion=...)")
        if grad_distortion.numel() != H * W or grad_distortion.ndim not in (2, 3):
            raise RuntimeError(f"grad_out_distortion must have shape (1, {H}, {W}), got {tuple(grad_distortion.shape)}")
        grad_distortion = grad_distortion.to(torch.float32).contiguous()
    if grad_median is not None:
        if getattr(st, "median", None) is None:
            raise RuntimeError("grad_out_median_depth needs a state from forward_raw(..., median_depth=True)")
        if grad_median.numel() != H * W or grad_median.ndim not in (2, 3):
            raise RuntimeError(f"grad_out_median_depth must have shape (1, {H}, {W}), got {tuple(grad_median.shape)}")
        grad_median = grad_median.to(torch.float32).contiguous()
    bg_image = _background(st.bg, H, W)
    ext = None
    if bg_image or grad_alpha is not None or dbg is not None:
        ext = _native.CompositeExt(background_image=_ptr(st.bg) if bg_image else None, dL_dalpha=_ptr(grad_alpha),
                                   dL_dbackground=None if bg_image else _ptr(dbg),
                                   dL_dbackground_image=_ptr(dbg) if bg_image else None)
    return _Upstream(grad_color, grad_depth, grad_alpha, grad_features, grad_distortion, grad_median, bg_image, ext)


def _backward_args(st: ForwardState, rs, up: _Upstream, accumulate_stats, **fields):
    """BackwardArgs with the fields every backward call shares -- the forward's inputs and buffers, the settings, the
    upstream gradients -- and `fields`: the call's stages, range and destinations."""
    return _native.BackwardArgs(
        P=st.radii.shape[0], D=int(rs.sh_degree), M=st.M, W=int(rs.image_width), H=int(rs.image_height),
        R=st.num_rendered, num_big=st.num_big, background=None if up.bg_image else _ptr(st.bg),
        means3D=_ptr(st.means3D), colors_precomp=_ptr(st.colors_precomp), opacities=_ptr(st.opacities),
        scales=_ptr(st.scales), scale_modifier=float(rs.scale_modifier), rotations=_ptr(st.rotations),
        cov3D_precomp=_ptr(st.cov3D_precomp), viewmatrix=_ptr(st.viewmatrix), projmatrix=_ptr(st.projmatrix),
        campos=_ptr(st.campos), tan_fovx=float(rs.tanfovx), tan_fovy=float(rs.tanfovy),
        dL_dpix=up.color.data_ptr(), dL_dinvdepth=_ptr(up.depth), shs=_ptr(st.shs),
        radii=_ptr(st.radii), geom_buffer=_ptr(st.geom_buffer), binning_buffer=_ptr(st.binning_buffer),
        image_buffer=_ptr(st.image_buffer), antialiasing=int(bool(rs.antialiasing)), debug=int(bool(rs.debug)),
        densify_accumulate=int(bool(accumulate_stats)), **fields)


def _absgrad_ext(dabs: torch.Tensor, abs_stats, n: int):
    """AbsgradExt for n Gaussians' destination dabs (n,2): an empty tensor's pointer is passed as NULL, and the library
    then writes nothing; abs_stats counts only with a Gaussian to write."""
    return _native.AbsgradExt(dL_dmeans2D_abs=_ptr(dabs), densify_abs=int(bool(abs_stats) and n > 0))


def backward_raw(state: ForwardState, raster_settings, grad_out_color, grad_out_depth=None, out=None,
                 compact_sh=False, accumulate_stats=False, camera_grads=False, grad_out_alpha=None,
                 background_grad=False, absgrad=False, abs_stats=False, grad_out_features=None,
                 grad_out_distortion=None, grad_out_median_depth=None):
    """One call of gsr_backward.  Returns a dict of gradients (means3D, means2D, shs, colors_precomp,
    opacities, scales, rotations, cov3D_precomp); entries are None where the input was absent.
    `out` may supply preallocated contiguous float32 destinations (e.g. views into one flat buffer that is
    then all-reduced): keys means2D (P,3), colors (P,3), opacities (P,1), means3D (P,3), cov3D (P,6),
    shs (P,M,3), scales (P,3), rotations (P,4), colors_sh (P,3), densify_stats (P,2) (|dL/dmeans2D[:2]| and
    radii > 0 of this view, gaussian_model.py:175-181), max_radii2D (P,) int32, and campos_rows = (rows (V,3),
    rank): the multi-view exchange's camera block, written by the backward (campos in row `rank`, zeros elsewhere).
    accumulate_stats=True adds this view's densify_stats to out["densify_stats"] (the reference's
    add_densification_stats); out["max_radii2D"] is always max-accumulated with this view's radii.
    compact_sh=True skips dL/dshs and returns the clamp-masked colour gradient "colors_sh" instead -- the
    per-view factor that `sh_backward_views` expands after an all-gather (multiview.py).
    camera_grads=True adds the gradients of the camera, as three independent inputs: viewmatrix (4,4) (column 3
    zero), projmatrix (4,4) (column 2 zero) and campos (3) (zero without SH colours); `out` may supply them under
    those names.  Deterministic sums over the Gaussians; the other gradients are bitwise what they are without.
    grad_out_alpha (1,H,W) or (H,W) is the upstream gradient of forward_raw's alpha.  background_grad=True adds "bg",
    the gradient of the background the forward composited over, in its shape -- (3,) (a fixed-order sum over the
    pixels, bitwise reproducible) or (3,H,W); `out` may supply it as out["bg"].  With a (3,H,W) background, an alpha
    gradient or background_grad the call is gsr_backward_ext; the Gaussians' gradients without an alpha gradient are
    bitwise those of the plain call.
    absgrad=True adds "means2D_abs" (P,2): per Gaussian the sum over its pixels of |what the pixel adds to
    means2D[:, :2]|, the AbsGS densification criterion (gsplat's absgrad), in means2D's units and under every upstream
    gradient of the call; exactly zero for a Gaussian that is culled or that no pixel takes, deterministic, and every
    other gradient keeps its bits.  `out` may supply it as out["means2D_abs"] (which also asks for it).
    abs_stats=True (needs out["densify_stats"]; implies absgrad) forms densify_stats[:, 0] from that vector,
    sqrt(x * x + y * y) with every operation rounded once, instead of from the signed gradient.  The call is then
    gsr_backward_abs.
    A state that carries features (forward_raw(..., features=f)) adds "features" (P,C), the gradient of f; `out` may
    supply it as out["features"].  grad_out_features (C,H,W) is the upstream gradient of the feature image: through
    alpha it also enters every other gradient of the call, which then is the joint gradient of colour, inverse depth,
    alpha and features.  With grad_out_features=None "features" is zeros and every other gradient has the bits of the
    call without features.  The call is then gsr_backward_features; absgrad / abs_stats with it raise
    NotImplementedError (the absolute sums of a joint call are not built).
    grad_out_distortion (1,H,W) or (H,W), for a state that carries distortion (forward_raw(..., distortion=...)), is
    the upstream gradient of the distortion map: through the weights and through the Gaussians' depths it enters every
    other gradient of the call, the camera's included, in a fixed summation order.  With grad_out_distortion=None
    every gradient has the bits of the call without distortion.  The call is then gsr_backward_distortion; absgrad /
    abs_stats with it raise NotImplementedError.
    grad_out_median_depth (1,H,W) or (H,W), for a state that carries the median (forward_raw(..., median_depth=True)),
    is the upstream gradient of median_depth.  The selection is piecewise constant: the gradient reaches only the depth
    of each pixel's selected Gaussian, and through it means3D and the camera, in a fixed summation order; opacities,
    scales, rotations, means2D and the colours get nothing from it.  With grad_out_median_depth=None every gradient
    has the bits of the call without the median.  The call is then gsr_backward_median; absgrad / abs_stats with it
    raise NotImplementedError."""
    if abs_stats and "densify_stats" not in (out or {}):
        raise RuntimeError("abs_stats=True needs out['densify_stats']")
    lib = _native.load()
    rs = raster_settings
    st = state
    device = st.radii.device  # (a scene without Gaussians keeps no means3D; its background gradients still exist)
    P = st.radii.shape[0]
    M = st.M
    f32 = dict(dtype=torch.float32, device=device)
    out = out or {}

    def dst(name, *shape):
        t = out.get(name)
        if t is None:
            return torch.empty(*shape, **f32)
        if tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous():
            raise RuntimeError(f"out[{name!r}] must be a contiguous float32 tensor of shape {shape}")
        return t

    dmeans2D = dst("means2D", P, 3)
    # dL/dcolors and dL/dcov3D are outputs only for precomputed colours / covariances (or when asked for)
    dcolors = dst("colors", P, 3) if (st.colors_precomp is not None or "colors" in out) else None
    dopac = dst("opacities", P, 1)
    dmeans3D = dst("means3D", P, 3)
    dcov = dst("cov3D", P, 6) if (st.cov3D_precomp is not None or "cov3D" in out) else None
    dsh = None if compact_sh else dst("shs", P, max(M, 0), 3)
    dcsh = dst("colors_sh", P, 3) if (compact_sh or "colors_sh" in out) else None
    dstats = dst("densify_stats", P, 2) if "densify_stats" in out else None
    dabs = dst("means2D_abs", P, 2) if (absgrad or abs_stats or "means2D_abs" in out) else None
    mrad = out.get("max_radii2D")
    if mrad is not None and (tuple(mrad.shape) != (P,) or mrad.dtype != torch.int32 or not mrad.is_contiguous()):
        raise RuntimeError(f"out['max_radii2D'] must be a contiguous int32 tensor of shape ({P},)")
    dscales = dst("scales", P, 3)
    drot = dst("rotations", P, 4)
    cam_rows, cam_rank, cam_n = _campos_rows(out.get("campos_rows"))
    dview = dst("viewmatrix", 4, 4) if camera_grads else None
    dproj = dst("projmatrix", 4, 4) if camera_grads else None
    dcampos = dst("campos", 3) if camera_grads else None
    dbg = dst("bg", *st.bg.shape) if (background_grad or "bg" in out) else None
    up = _upstream(st, rs, grad_out_color, grad_out_depth, grad_out_alpha, grad_out_features, dbg,
                   grad_out_distortion, grad_out_median_depth)
    feat = dfeat = None
    if st.features is not None:
        C = int(st.features.shape[1])
        dfeat = dst("features", P, C)
        feat = _native.FeaturesExt(C=C, features=_ptr(st.features), dL_dout_features=_ptr(up.features),
                                   dL_dfeatures=_ptr(dfeat))
    dist = None
    ds = getattr(st, "distortion", None)
    if ds is not None:
        dist = _native.DistortionExt(map=_native.DISTORTION_MAPS[ds.map], near_plane=ds.near, far_plane=ds.far,
                                     total_weight=ds.totals[0].data_ptr(), total_moment=ds.totals[1].data_ptr(),
                                     dL_ddistortion=_ptr(up.distortion))
    med = None
    ms = getattr(st, "median", None)
    if ms is not None:
        med = _native.MedianExt(median_pos=ms.pos.data_ptr(), dL_dmedian_depth=_ptr(up.median))
    # (features, distortion or the median with absgrad: refused by the library, GSR_ERR_UNSUPPORTED ->
    # NotImplementedError)
    ab = None if dabs is None else _absgrad_ext(dabs, abs_stats, P)
    bufs = _Buffers(device)
    a = _backward_args(
        st, rs, up, accumulate_stats,
        dL_dmeans2D=dmeans2D.data_ptr(), dL_dcolors=_ptr(dcolors), dL_dopacity=dopac.data_ptr(),
        dL_dmeans3D=dmeans3D.data_ptr(), dL_dcov3D=_ptr(dcov), dL_dsh=_ptr(dsh),
        dL_dscales=dscales.data_ptr(), dL_drotations=drot.data_ptr(), dL_dcolors_sh=_ptr(dcsh),
        densify_stats=_ptr(dstats), max_radii2D=_ptr(mrad),
        campos_rows=cam_rows, campos_rank=cam_rank, campos_nrows=cam_n,
        dL_dviewmatrix=_ptr(dview), dL_dprojmatrix=_ptr(dproj), dL_dcampos=_ptr(dcampos))
    with torch.cuda.device(device):
        rc = _native.call_backward(lib, a, ext=up.ext, absgrad=ab, feat=feat, cb=bufs.callback,
                                   stream=_stream_handle(device), dist=dist, median=med)
    bufs.raise_pending()
    _native.check(rc, "rasterize_gaussians_backward")
    camera = dict(viewmatrix=dview, projmatrix=dproj, campos=dcampos) if camera_grads else {}
    if dbg is not None:
        camera["bg"] = dbg
    if dabs is not None:
        camera["means2D_abs"] = dabs
    if dfeat is not None:
        camera["features"] = dfeat
    return dict(
        **camera,
        means3D=dmeans3D, means2D=dmeans2D,
        shs=dsh.view_as(st.shs) if (st.shs is not None and dsh is not None) else None, colors_sh=dcsh,
        colors_precomp=dcolors if st.colors_precomp is not None else None,
        colors=dcolors, opacities=dopac.view_as(st.opacities) if st.opacities is not None else dopac,
        scales=dscales if st.scales is not None else None,
        rotations=drot if st.rotations is not None else None,
        cov3D_precomp=dcov if st.cov3D_precomp is not None else None, cov3D=dcov)


def _pixel_weights(pixel_weights, H: int, W: int, device):
    """The weight image as a contiguous float32 (H,W) tensor on the device (None stays None); RuntimeError otherwise."""
    if pixel_weights is None:
        return None
    if not torch.is_tensor(pixel_weights) or tuple(pixel_weights.shape) not in ((H, W), (1, H, W)):
        raise RuntimeError(f"pixel_weights must have shape ({H}, {W}) or (1, {H}, {W}), got "
                           f"{tuple(pixel_weights.shape) if torch.is_tensor(pixel_weights) else type(pixel_weights).__name__}")
    if pixel_weights.dtype != torch.float32:
        raise RuntimeError(f"pixel_weights must be float32 (got {pixel_weights.dtype})")
    if pixel_weights.device != device:
        pixel_weights = pixel_weights.to(device)
    return pixel_weights.detach().reshape(H, W).contiguous()


_CONTRIB_DTYPES = dict(count=torch.int64, wsum=torch.float32, wmax=torch.float32)


def contributions_raw(state: ForwardState, raster_settings, pixel_weights=None, out=None, accumulate=False):
    """One call of gsr_contributions on a forward's state: per Gaussian, over the (Gaussian, pixel) pairs the colour
    forward composited, dict(count (P,) int64, wsum (P,) float32, wmax (P,) float32) -- the number of pairs, and the
    sum and the max of the compositing weight w = alpha T, the colour render's own.  What pruning and budgeting
    methods reduce over views (LightGaussian: wsum, RadSplat: wmax, Mini-Splatting / Taming-3DGS: count).
    pixel_weights (H,W) or (1,H,W) float32: the pair's value is m(pix) * w instead (error-based densification), and a
    pixel whose m is not > 0 is left out of all three.  Exactly 0 for a Gaussian that is culled or that no pixel
    takes; deterministic (no float atomics); the state is only read, so a backward_raw after it has the bits it has
    without.  `out` may supply any of the three as contiguous (P,) tensors of those dtypes: then only those are
    produced (the others are None in the result), so each can be asked for alone.  accumulate=True adds this view to
    the buffers in `out` (count +=, wsum = wsum + this view's sum, wmax = max) and needs `out`."""
    rs, st = raster_settings, state
    device = st.radii.device
    P = int(st.radii.shape[0])
    H, W = int(rs.image_height), int(rs.image_width)
    out = dict(out or {})
    for name in out:
        if name not in _CONTRIB_DTYPES:
            raise RuntimeError(f"out[{name!r}]: the outputs are count, wsum and wmax")
    if accumulate and not out:
        raise RuntimeError("accumulate=True needs the buffers to add to in out")
    res = dict.fromkeys(_CONTRIB_DTYPES)  # with `out`, the entries it does not hold stay None: not produced
    for name, dtype in _CONTRIB_DTYPES.items():
        t = out.get(name)
        if t is None:
            continue
        if not torch.is_tensor(t) or tuple(t.shape) != (P,) or t.dtype != dtype or not t.is_contiguous():
            raise RuntimeError(f"out[{name!r}] must be a contiguous {dtype} tensor of shape ({P},)")
        if t.device != device:
            raise RuntimeError(f"out[{name!r}] must be on {device}")
        res[name] = t
    m = _pixel_weights(pixel_weights, H, W, device)
    if device.type != "cuda":
        raise RuntimeError("the MI355X rasterizer needs its inputs on a HIP device (tensor.device.type == 'cuda')")
    lib = _native.load()
    if not out:
        res = {name: torch.empty(P, dtype=dtype, device=device) for name, dtype in _CONTRIB_DTYPES.items()}
    bufs = _Buffers(device)
    a = _native.ContribArgs(P=P, W=W, H=H, R=st.num_rendered, num_big=st.num_big, radii=_ptr(st.radii),
                            geom_buffer=_ptr(st.geom_buffer), binning_buffer=_ptr(st.binning_buffer),
                            image_buffer=_ptr(st.image_buffer), pixel_weights=_ptr(m), count=_ptr(res["count"]),
                            wsum=_ptr(res["wsum"]), wmax=_ptr(res["wmax"]), accumulate=int(bool(accumulate)))
    if P:
        with torch.cuda.device(device):
            rc = _native.call_contributions(lib, a, bufs.callback, _stream_handle(device))
        bufs.raise_pending()
        _native.check(rc, "rasterize_contributions")
    return res


def backward_chunked(state: ForwardState, raster_settings, grad_out_color, grad_out_depth, chunks, on_chunk=None,
                     compact_sh=False, accumulate_stats=False, after_composite=None, grad_out_alpha=None,
                     bg_out=None, abs_stats=False):
    """The backward split so that a gradient exchange overlaps it (multiview.py): ONE gsr_backward call for the
    compositing backward (GSR_BWD_COMPOSITE: instance gradient rows into a scratch buffer kept here), then one call
    per Gaussian chunk for the per-Gaussian stage (GSR_BWD_GAUSSIANS), each followed by on_chunk(k) -- which may
    issue collectives on the chunk's finished gradients while the next chunks compute.

    chunks: list of (g_begin, g_end, out) with out a dict of destinations for those Gaussians only (same keys and
    row widths as backward_raw's `out`, (g_end - g_begin) rows each, contiguous float32; max_radii2D int32).
    Results are bitwise those of one backward_raw call: every Gaussian is computed by the same code.
    A chunk's out may also hold viewmatrix (4,4), projmatrix (4,4) and campos (3): the camera gradients summed over
    that chunk's Gaussians (the caller adds the chunks; each chunk needs its own destinations).
    after_composite(), when given, runs between the compositing call and the first per-Gaussian call.
    grad_out_alpha: the upstream gradient of alpha, read by the compositing call (as backward_raw's); bg_out: a
    contiguous float32 destination shaped like the background, which the compositing call fills with its gradient
    (backward_raw's "bg").
    A chunk's out may hold means2D_abs ((g_end - g_begin), 2), backward_raw's "means2D_abs" for those Gaussians: then
    every chunk must, since the compositing call produces the rows they are summed from.  abs_stats=True forms each
    chunk's densify_stats[:, 0] from it (every chunk then needs both).
    A state that carries features raises NotImplementedError: the split backward of feature channels is not built;
    so does a state that carries distortion or the median depth."""
    lib = _native.load()
    rs = raster_settings
    st = state
    if getattr(st, "distortion", None) is not None:
        raise NotImplementedError("backward_chunked: a forward state with distortion needs backward_raw (the split "
                                  "backward of the distortion map is not built)")
    if getattr(st, "median", None) is not None:
        raise NotImplementedError("backward_chunked: a forward state with the median depth needs backward_raw (the "
                                  "split backward of the median depth is not built)")
    if st.features is not None:
        raise NotImplementedError("backward_chunked: a forward state with features needs backward_raw (the split "
                                  "backward of feature channels is not built)")
    device = st.radii.device  # (as backward_raw: a scene without Gaussians keeps no means3D)
    M = st.M
    if bg_out is not None and (tuple(bg_out.shape) != tuple(st.bg.shape) or bg_out.dtype != torch.float32
                               or not bg_out.is_contiguous()):
        raise RuntimeError(f"bg_out must be a contiguous float32 tensor of shape {tuple(st.bg.shape)}")
    # (the per-Gaussian calls take up.ext too: with a background image there is no background vector)
    up = _upstream(st, rs, grad_out_color, grad_out_depth, grad_out_alpha, dbg=bg_out)

    chunks = list(chunks)
    with_abs = [("means2D_abs" in out) for _, _, out in chunks]
    if any(with_abs) and not all(with_abs):
        raise RuntimeError("means2D_abs must be in every chunk's out or in none")
    if abs_stats and not (chunks and all(with_abs) and all("densify_stats" in out for _, _, out in chunks)):
        raise RuntimeError("abs_stats=True needs out['means2D_abs'] and out['densify_stats'] in every chunk")

    def call(a, ab=None):
        return _native.call_backward(lib, a, ext=up.ext, absgrad=ab, feat=None, cb=bufs.callback,
                                     stream=_stream_handle(device))

    bufs = _Buffers(device)
    with torch.cuda.device(device):
        a = _backward_args(st, rs, up, accumulate_stats, stages=_native.GSR_BWD_COMPOSITE)
        # (the compositing call does not write through the pointer: non-NULL asks for the abs rows)
        want_abs = any(with_abs) and any(out["means2D_abs"].numel() for _, _, out in chunks)
        rc = call(a, _absgrad_ext(next(out["means2D_abs"] for _, _, out in chunks if out["means2D_abs"].numel()),
                                  False, 0) if want_abs else None)
        bufs.raise_pending()
        _native.check(rc, "rasterize_gaussians_backward (composite)")
        scratch = bufs.get(_native.GSR_BUF_BWD_SCRATCH)
        if after_composite is not None:
            after_composite()
        widths = dict(means2D=3, colors=3, opacities=1, means3D=3, cov3D=6, shs=3 * max(M, 0), scales=3, rotations=4,
                      colors_sh=3, densify_stats=2, means2D_abs=2)
        for k, (g0, g1, out) in enumerate(chunks):
            n = int(g1) - int(g0)
            cam_rows, cam_rank, cam_n = _campos_rows(out.get("campos_rows"))
            for name, t in out.items():
                if name == "campos_rows":
                    continue
                if name in _CAMERA_SHAPES:
                    if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != _CAMERA_SHAPES[name]:
                        raise RuntimeError(f"chunk {k}: out[{name!r}] must be a contiguous float32 tensor of shape "
                                           f"{_CAMERA_SHAPES[name]}")
                    continue
                want = (torch.int32, (n,)) if name == "max_radii2D" else (torch.float32, None)
                if t.dtype != want[0] or not t.is_contiguous() or t.shape[0] != n or (
                        name in widths and t.numel() != n * widths[name]):
                    raise RuntimeError(f"chunk {k}: out[{name!r}] must be a contiguous {want[0]} tensor of {n} rows")
            if compact_sh and "colors_sh" not in out and st.shs is not None:
                raise RuntimeError("compact_sh needs out['colors_sh'] in every chunk")
            a = _backward_args(
                st, rs, up, accumulate_stats, stages=_native.GSR_BWD_GAUSSIANS, g_begin=int(g0), g_end=int(g1), bwd_scratch=_ptr(scratch),
                dL_dmeans2D=_ptr(out.get("means2D")), dL_dcolors=_ptr(out.get("colors")),
                dL_dopacity=_ptr(out.get("opacities")), dL_dmeans3D=_ptr(out.get("means3D")),
                dL_dcov3D=_ptr(out.get("cov3D")), dL_dsh=None if compact_sh else _ptr(out.get("shs")),
                dL_dscales=_ptr(out.get("scales")), dL_drotations=_ptr(out.get("rotations")),
                dL_dcolors_sh=_ptr(out.get("colors_sh")), densify_stats=_ptr(out.get("densify_stats")),
                max_radii2D=_ptr(out.get("max_radii2D")), campos_rows=cam_rows, campos_rank=cam_rank,
                campos_nrows=cam_n, dL_dviewmatrix=_ptr(out.get("viewmatrix")),
                dL_dprojmatrix=_ptr(out.get("projmatrix")), dL_dcampos=_ptr(out.get("campos")))
            rc = call(a, _absgrad_ext(out["means2D_abs"], abs_stats, n) if want_abs else None)
            bufs.raise_pending()
            _native.check(rc, f"rasterize_gaussians_backward (chunk {k})")
            if on_chunk is not None:
                on_chunk(k)
    return scratch


_CAMERA_SHAPES = dict(viewmatrix=(4, 4), projmatrix=(4, 4), campos=(3,))


def _campos_rows(spec):
    """(pointer, rank, rows) of an out["campos_rows"] = (rows (V, 3) contiguous float32, rank) entry."""
    if spec is None:
        return None, 0, 0
    rows, rank = spec
    if rows.dtype != torch.float32 or not rows.is_contiguous() or rows.ndim != 2 or rows.shape[1] != 3:
        raise RuntimeError("out['campos_rows'] must be (contiguous float32 (V, 3) tensor, rank)")
    if not 0 <= int(rank) < rows.shape[0]:
        raise RuntimeError(f"campos_rows rank {rank} outside [0, {rows.shape[0]})")
    return rows.data_ptr(), int(rank), int(rows.shape[0])


def _save_state(ctx, st: ForwardState):
    """Keep a ForwardState on an autograd context: its tensors saved (an empty one in place of None), the rest plain."""
    ds = getattr(st, "distortion", None)
    ms = getattr(st, "median", None)
    tensors = (st[:15] + (() if st.features is None else (st.features,)) + (() if ds is None else (ds.totals,))
               + (() if ms is None else (ms.pos,)))
    ctx.has_median = ms is not None
    ctx.meta = (st.num_rendered, st.num_big, st.M)
    ctx.has_features = st.features is not None
    ctx.distortion = None if ds is None else tuple(ds[:3])
    ctx.present = tuple(t is not None for t in tensors)
    empty = torch.empty(0, device=st.radii.device)
    ctx.save_for_backward(*[(t if t is not None else empty) for t in tensors])


def _saved_state(ctx) -> ForwardState:
    tensors = [t if present else None for t, present in zip(ctx.saved_tensors, ctx.present)]
    extra = tensors[15:]
    features = extra.pop(0) if ctx.has_features else None
    if ctx.distortion is None and not ctx.has_median:
        return ForwardState(*tensors[:15], *ctx.meta, features)
    st = _ExtendedForwardState(*tensors[:15], *ctx.meta, features)
    if ctx.distortion is not None:
        st.distortion = DistortionState(*ctx.distortion, extra.pop(0))
    if ctx.has_median:
        st.median = MedianState(extra.pop(0))
    return st


class _RasterizeGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                raster_settings, flags=(False, False), features=None, bg=None, *camera):
        # flags: (return_alpha, absgrad[, distortion: None or (map, near, far)[, median_depth]]).  features: None or the (P,C) channels.  bg: None or the settings' bg once
        # more, camera: () or the settings' (viewmatrix, projmatrix, campos) once more, as inputs autograd can hand a
        # gradient to (rasterize_gaussians); the values are read from the settings either way
        return_alpha, absgrad = flags[:2]
        dmap, dnear, dfar = (flags[2] if len(flags) > 2 and flags[2] is not None else (None, None, None))
        median_depth = len(flags) > 3 and bool(flags[3])
        res = forward_raw(means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings,
                          return_alpha=return_alpha, features=features, distortion=dmap, distortion_near=dnear,
                          distortion_far=dfar, median_depth=median_depth)
        ctx.raster_settings = raster_settings
        ctx.return_alpha = bool(return_alpha)
        # absgrad: the backward sets means2D.absgrad on the caller's tensor (as gsplat's does)
        ctx.absgrad_of = means2D if (absgrad and torch.is_tensor(means2D)) else None
        ctx.bg = None if bg is None else (tuple(bg.shape), bg.device)
        ctx.camera = [(tuple(t.shape), t.device) for t in camera]
        _save_state(ctx, res[-1])
        ctx.set_materialize_grads(False)
        if median_depth:
            ctx.mark_non_differentiable(res[-2])  # median_index
        return res[:-1]  # (color, radii, invdepth[, alpha][, feature_image][, distortion][, median_depth, median_index])

    @staticmethod
    def backward(ctx, grad_out_color, _grad_radii, grad_out_depth, *rest):
        st = _saved_state(ctx)
        rest = list(rest)
        grad_out_alpha = rest.pop(0) if ctx.return_alpha else None
        grad_out_features = rest.pop(0) if st.features is not None else None
        grad_out_distortion = rest.pop(0) if getattr(st, "distortion", None) is not None else None
        grad_out_median = rest.pop(0) if getattr(st, "median", None) is not None else None  # (then the index's: None)
        need = ctx.needs_input_grad
        g = backward_raw(st, ctx.raster_settings, grad_out_color, grad_out_depth, camera_grads=any(need[12:]),
                         grad_out_alpha=grad_out_alpha, background_grad=need[11], absgrad=ctx.absgrad_of is not None,
                         grad_out_features=grad_out_features, grad_out_distortion=grad_out_distortion,
                         grad_out_median_depth=grad_out_median)
        if ctx.absgrad_of is not None:  # (P,3) with z = 0, so code that takes [:, :2] of means2D.grad works on it
            m2a = g["means2D_abs"]
            ctx.absgrad_of.absgrad = torch.cat([m2a, m2a.new_zeros(m2a.shape[0], 1)], dim=1)
        camera = tuple(g[name].reshape(shape).to(dev) if wanted else None for name, (shape, dev), wanted in
                       zip(("viewmatrix", "projmatrix", "campos"), ctx.camera, need[12:]))
        return (g["means3D"] if need[0] else None,
                g["means2D"] if need[1] else None,
                g["shs"] if need[2] else None,
                g["colors_precomp"] if need[3] else None,
                g["opacities"] if need[4] else None,
                g["scales"] if need[5] else None,
                g["rotations"] if need[6] else None,
                g["cov3D_precomp"] if need[7] else None,
                None, None,  # raster_settings, flags
                g["features"] if need[10] else None,
                g["bg"].reshape(ctx.bg[0]).to(ctx.bg[1]) if need[11] else None,
                *camera)


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                        raster_settings, return_alpha=False, absgrad=False, features=None, distortion=None,
                        distortion_near=None, distortion_far=None, median_depth=False):
    """Differentiable with respect to the Gaussians' tensors and, where raster_settings.viewmatrix, .projmatrix or
    .campos requires grad, to those three as independent inputs (projmatrix being the full view-projection product:
    a caller optimising a pose builds projmatrix and campos from its view matrix in torch, which chains the three).
    raster_settings.bg -- (3,) or a (3,H,W) image -- receives its gradient too where it requires grad.
    return_alpha=True returns (color, radii, invdepth, alpha (1,H,W)) with alpha = 1 - the transmittance left behind
    each pixel's last contributor; alpha takes part in autograd like color and invdepth.  return_alpha (or an image
    bg) does not change color, except with no Gaussian at all (P == 0): the plain call then returns zeros like
    upstream, this one the background (forward_raw).
    absgrad=True: the backward also sets means2D.absgrad (P,3) = (sum over the Gaussian's pixels of |the pixel's
    contribution to means2D.grad[:, :2]|, 0), the AbsGS densification criterion, as gsplat's absgrad does; it is
    assigned (not accumulated) by every backward, and means2D.grad is what it is without.
    features (P,C), 1 <= C <= 64: the call returns (color, radii, invdepth[, alpha], feature_image (C,H,W)) with
    feature_image = sum_i alpha_i T_i features[i] -- the colour's weights, no background.  It takes part in autograd:
    features.grad is populated, and a loss on it reaches means3D, opacities, scales, rotations and the camera through
    alpha.  With absgrad=True it raises NotImplementedError (the absolute sums of a joint call are not built).
    distortion "z" or "ndc" (with distortion_near, distortion_far): the call's last output is the depth distortion map
    (1,H,W) = sum_i sum_j w_i w_j |t_i - t_j| (forward_raw).  It takes part in autograd: a loss on it reaches means3D,
    opacities, scales, rotations, means2D.grad and the camera.  With absgrad=True it raises NotImplementedError.
    median_depth=True: the call's last two outputs are median_depth (1,H,W) and median_index (1,H,W) int32
    (forward_raw).  median_depth takes part in autograd: a loss on it reaches means3D and the camera through the
    selected Gaussians' depths, and nothing else; median_index is not differentiable.  With absgrad=True it raises
    NotImplementedError."""
    if features is not None and absgrad:
        raise NotImplementedError("features with absgrad=True are not built yet")
    dist_spec = _distortion(distortion, distortion_near, distortion_far)
    if dist_spec is not None and absgrad:
        raise NotImplementedError("distortion with absgrad=True is not built")
    if median_depth and absgrad:
        raise NotImplementedError("median_depth with absgrad=True is not built")
    rs = raster_settings
    camera = (rs.viewmatrix, rs.projmatrix, rs.campos)
    if not (torch.is_grad_enabled() and all(torch.is_tensor(t) for t in camera)
            and any(t.requires_grad for t in camera)):
        camera = ()  # the call as it is without camera gradients
    bg = rs.bg if (torch.is_grad_enabled() and torch.is_tensor(rs.bg) and rs.bg.requires_grad) else None
    return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                                     cov3Ds_precomp, raster_settings,
                                     (bool(return_alpha), bool(absgrad)) + ((dist_spec, True) if median_depth else
                                                                            () if dist_spec is None else (dist_spec,)),
                                     features, bg, *camera)


@torch.no_grad()
def rasterize_contributions(means3D, opacities, raster_settings, shs=None, colors_precomp=None, scales=None,
                            rotations=None, cov3D_precomp=None, pixel_weights=None, out=None, accumulate=False):
    """One forward_raw, then contributions_raw on its state: (dict(count, wsum, wmax), radii).  Colours do not enter
    the weights: with neither shs nor colors_precomp the forward renders a zero (P,3) colors_precomp."""
    if shs is not None and colors_precomp is not None:
        raise Exception("Please provide at most one of either SHs or precomputed colors!")
    if ((scales is None or rotations is None) and cov3D_precomp is None) or (
            (scales is not None or rotations is not None) and cov3D_precomp is not None):
        raise Exception("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!")
    if shs is None and colors_precomp is None:
        colors_precomp = torch.zeros(means3D.shape[0], 3, dtype=torch.float32, device=means3D.device)
    res = forward_raw(means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, raster_settings)
    radii, state = res[1], res[-1]
    return contributions_raw(state, raster_settings, pixel_weights=pixel_weights, out=out, accumulate=accumulate), radii


def sh_backward_views(means3D: torch.Tensor, campos: torch.Tensor, dcolors_sh: torch.Tensor, sh_degree: int, M: int,
                      out: Optional[torch.Tensor] = None, chunk_len: int = 0) -> torch.Tensor:
    """dL/dshs (P,M,3) summed over V views from the compact per-view factors: campos (V,3) and the clamp-masked
    colour gradients dcolors_sh (V,P,3) that backward_raw(..., compact_sh=True) returns (gsr_sh_backward_views).
    chunk_len > 0: dcolors_sh is the flat chunk-major layout of multiview.py's chunked gather -- chunk c covers
    Gaussians [c*chunk_len, min(P, (c+1)*chunk_len)) as a (V, L_c, 3) block (gsr_sh_backward_views_chunked)."""
    lib = _native.load()
    device = means3D.device
    m = _prep(means3D, device, "means3D")
    c = _prep(campos, device, "campos").reshape(-1, 3)
    d = _prep(dcolors_sh, device, "dcolors_sh")
    P, V = m.shape[0], c.shape[0]
    if chunk_len and chunk_len < P:
        if d.numel() != V * P * 3:
            raise RuntimeError(f"chunked dcolors_sh must hold {V * P * 3} floats, got {d.numel()}")
    elif tuple(d.shape) != (V, P, 3):
        raise RuntimeError(f"dcolors_sh must have shape {(V, P, 3)}, got {tuple(d.shape)}")
    if out is None:
        out = torch.empty(P, M, 3, dtype=torch.float32, device=device)
    elif tuple(out.shape) != (P, M, 3) or out.dtype != torch.float32 or not out.is_contiguous():
        raise RuntimeError(f"out must be a contiguous float32 tensor of shape {(P, M, 3)}")
    with torch.cuda.device(device):
        rc = lib.gsr_sh_backward_views_chunked(P, int(sh_degree), int(M), V, int(chunk_len), _ptr(m), _ptr(c), _ptr(d),
                                               out.data_ptr(), _stream_handle(device))
    _native.check(rc, "sh_backward_views")
    return out


def mark_visible(positions: torch.Tensor, viewmatrix: torch.Tensor, projmatrix: torch.Tensor) -> torch.Tensor:
    lib = _native.load()
    device = positions.device
    pos = _prep(positions, device, "positions")
    view = _prep(viewmatrix, device, "viewmatrix")
    proj = _prep(projmatrix, device, "projmatrix")
    P = positions.shape[0]
    present = torch.zeros(P, dtype=torch.bool, device=device)
    if P:
        with torch.cuda.device(device):
            rc = lib.gsr_mark_visible(P, _ptr(pos), _ptr(view), _ptr(proj), present.data_ptr(),
                                      _stream_handle(device))
        _native.check(rc, "mark_visible")
    return present


class GaussianRasterizer(nn.Module):
    def __init__(self, raster_settings: GaussianRasterizationSettings, return_alpha: bool = False,
                 absgrad: bool = False, distortion: Optional[str] = None, distortion_near: Optional[float] = None,
                 distortion_far: Optional[float] = None, median_depth: bool = False):
        """return_alpha=True: the call returns (color, radii, invdepth, alpha (1,H,W)); with P == 0 its color is the
        background where the plain call's is zero (rasterize_gaussians).  absgrad=True: the backward sets
        means2D.absgrad (rasterize_gaussians).  distortion="z" or "ndc" (with distortion_near, distortion_far): the
        call's last output is the depth distortion map (1,H,W) (rasterize_gaussians).  median_depth=True: the call's
        last two outputs are median_depth (1,H,W) and median_index (1,H,W) int32 (rasterize_gaussians)."""
        super().__init__()
        self.median_depth = bool(median_depth)
        self.distortion = _distortion(distortion, distortion_near, distortion_far)
        self.raster_settings = raster_settings
        self.return_alpha = bool(return_alpha)
        self.absgrad = bool(absgrad)

    def markVisible(self, positions: torch.Tensor) -> torch.Tensor:
        with torch.no_grad():
            rs = self.raster_settings
            return mark_visible(positions, rs.viewmatrix, rs.projmatrix)

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None, features=None):
        rs = self.raster_settings
        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
            raise Exception("Please provide excatly one of either SHs or precomputed colors!")
        if ((scales is None or rotations is None) and cov3D_precomp is None) or (
                (scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!")
        # (color, radii, invdepth[, alpha][, feature_image (C,H,W)][, distortion (1,H,W)][, median_depth (1,H,W),
        # median_index (1,H,W)]): rasterize_gaussians
        dmap, dnear, dfar = self.distortion or (None, None, None)
        return rasterize_gaussians(means3D, means2D, shs, colors_precomp, opacities, scales, rotations,
                                   cov3D_precomp, rs, return_alpha=self.return_alpha, absgrad=self.absgrad,
                                   features=features, distortion=dmap, distortion_near=dnear, distortion_far=dfar,
                                   median_depth=self.median_depth)

    def contributions(self, means3D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                      cov3D_precomp=None, pixel_weights=None, out=None, accumulate=False):
        """(dict(count, wsum, wmax), radii) of this view: the per-Gaussian hit count and the sum and max of the
        compositing weight, without a gradient (rasterize_contributions, contributions_raw)."""
        return rasterize_contributions(means3D, opacities, self.raster_settings, shs=shs,
                                       colors_precomp=colors_precomp, scales=scales, rotations=rotations,
                                       cov3D_precomp=cov3D_precomp, pixel_weights=pixel_weights, out=out,
                                       accumulate=accumulate)
