"""Densification (prune / clone / split) on the HIP kernels of csrc/gsr_densify.hip.

Mirrors the reference's adaptive density control:

* `update_max_radii2D` / `update_xyz_gradient` -- gs_lightning/modules/gaussian_model.py:175-181;
* `densify_and_prune`  -- gaussian_model.py:184-287 (prune by opacity / screen size / world size, then clone
  small and split large Gaussians whose mean screen-space gradient reaches the threshold);
* with `optimizer=` also `update_optimizer_parameters` of gs_lightning/lightning/gs_lightning_module.py:213-235
  (Adam moments re-indexed with the kept rows, zero rows appended for the new Gaussians).

`gaussians` is any object with the reference GaussianModel's attributes: `_xyz (N,3)`, `_features_dc (N,1,3)`,
`_features_rest (N,K,3)`, `_opacity (N,1)`, `_scaling (N,3)`, `_rotation (N,4)`, `xyz_grad_accum (N)`,
`xyz_grad_count (N)`, `max_radii2D (N)`, `spatial_scale` and `use_screensize_threshold`.  All parameters and
moments move in one scatter launch; the only host sync is the read-back of the three row counts, which sizes
the outputs.  The split displacement is drawn as `normal_(0, 1)` of shape (n_split, 3) on the parameters'
device -- the same draw `torch.normal(mean, std)` makes -- so with the same generator state the result matches
the reference row for row.  No CPU fallback: the HIP library must load.

The second strategy, 3DGS-MCMC (csrc/gsr_mcmc.hip), is at the end of the file: `inject_noise`, `relocate_dead`,
`add_new` and `mcmc_relocation`.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn

from . import _native
from .rasterizer import _stream_handle

__all__ = ["PARAMETER_NAMES", "update_max_radii2D", "update_xyz_gradient", "densify_and_prune", "prune_points",
           "accumulate_contributions", "reset_contributions", "prune_by_contribution",
           "mcmc_relocation", "inject_noise", "relocate_dead", "add_new"]

PARAMETER_NAMES = ("xyz", "features_dc", "features_rest", "opacity", "scaling", "rotation")
_KINDS = dict(xyz=_native.FIELD_XYZ, scaling=_native.FIELD_SCALING)
_STATS = ("max_radii2D", "xyz_grad_accum", "xyz_grad_count")


@torch.no_grad()
def update_max_radii2D(gaussians, radii: torch.Tensor, visible_mask: torch.Tensor) -> None:
    """gaussian_model.py:175-176."""
    gaussians.max_radii2D[visible_mask] = torch.max(gaussians.max_radii2D[visible_mask],
                                                    radii[visible_mask].to(gaussians.max_radii2D.dtype))


@torch.no_grad()
def update_xyz_gradient(gaussians, screenspace_gradient: torch.Tensor, visible_mask: torch.Tensor,
                        absgrad: torch.Tensor = None) -> None:
    """gaussian_model.py:178-181.  absgrad, when given (means2D.absgrad of a rasterizer built with absgrad=True, or
    backward_raw's "means2D_abs"; (P,2) or (P,3)), is accumulated in place of screenspace_gradient: the AbsGS
    criterion, under which a large Gaussian whose per-pixel gradients cancel is still split.  Its norm is never below
    the signed one (4-6x above it on this repository's test scenes), and the reference's densify_grad_threshold is not
    retuned here: a caller that switches it on clones and splits more at the same threshold, and is expected to raise
    the threshold (AbsGS and gsplat use about twice the signed default)."""
    if absgrad is not None:
        screenspace_gradient = absgrad
    gaussians.xyz_grad_accum[visible_mask] += torch.norm(screenspace_gradient[visible_mask, :2], dim=1)
    gaussians.xyz_grad_count[visible_mask] += 1


def _f32(t: torch.Tensor) -> torch.Tensor:
    t = t.detach()
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def _group_for(optimizer, name: str, param):
    for group in optimizer.param_groups:
        if group.get("name", None) == name:
            if len(group["params"]) != 1:
                raise RuntimeError(f"param group {name!r} must hold exactly one tensor")
            return group
    return None


def _scatter_and_rebind(lib, gaussians, params, stats, optimizer, ws, z, N: int, n_new: int, stream) -> None:
    """The tail densify_and_prune and prune_points share: scatter every field (parameters, Adam moments, the three
    densification statistics) through the classified workspace `ws` into arrays of n_new rows (gsr_densify_apply), then
    rebind them on `gaussians` and in the optimizer.  z: the (n_split, 3) normal draws (empty without splits)."""
    dev = params["xyz"].device
    fields, new_params, new_states, moved = [], {}, {}, {}
    for k in PARAMETER_NAMES:
        src = params[k]
        dst = torch.empty((n_new,) + tuple(src.shape[1:]), dtype=torch.float32, device=dev)
        new_params[k] = dst
        width = src[0].numel() if N else 0
        m_src = v_src = m_dst = v_dst = None
        if optimizer is not None:
            group = _group_for(optimizer, k, src)
            st = optimizer.state.get(group["params"][0], None) if group is not None else None
            if st is not None and "exp_avg" in st:
                m_src, v_src = st["exp_avg"].contiguous(), st["exp_avg_sq"].contiguous()
                m_dst, v_dst = torch.empty_like(dst), torch.empty_like(dst)
                new_states[k] = (group, st, m_dst, v_dst)
                moved[k] = (m_src, v_src)
            elif group is not None:
                new_states[k] = (group, None, None, None)
        if width:
            ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
            fields.append(_native.DensifyField(src.data_ptr(), dst.data_ptr(), ptr(m_src), ptr(v_src), ptr(m_dst),
                                               ptr(v_dst), width, _KINDS.get(k, _native.FIELD_PLAIN)))
    new_stats = {}
    for k in _STATS:
        dst = torch.empty(n_new, dtype=torch.float32, device=dev)
        new_stats[k] = dst
        fields.append(_native.DensifyField(stats[k].data_ptr(), dst.data_ptr(), None, None, None, None, 1,
                                           _native.FIELD_STAT))
    arr = (_native.DensifyField * len(fields))(*fields)
    if n_new:
        _native.check(lib.gsr_densify_apply(N, ws.data_ptr(), params["rotation"].data_ptr(),
                                            params["scaling"].data_ptr(), z.data_ptr(), arr, len(fields), stream),
                      "gsr_densify_apply")
    _drop_contributions(gaussians)  # (N, ...) buffers of the rows that were: every change of N drops them

    _rebind(gaussians, optimizer, new_params, new_stats, new_states)


def _rebind(gaussians, optimizer, new_params, new_stats, new_states) -> None:
    """Rebind exactly as the reference does (nn.Parameter per attribute; optimizer state moved to the new key)."""
    for k in PARAMETER_NAMES:
        setattr(gaussians, f"_{k}", nn.Parameter(new_params[k]))
    for k in _STATS:
        old = getattr(gaussians, k)
        setattr(gaussians, k, new_stats[k].to(old.dtype))
    for k, (group, st, m_dst, v_dst) in new_states.items():
        old_p = group["params"][0]
        new_p = getattr(gaussians, f"_{k}")
        if st is not None:
            st["exp_avg"], st["exp_avg_sq"] = m_dst, v_dst
            del optimizer.state[old_p]
            group["params"][0] = new_p
            optimizer.state[new_p] = st
        else:
            group["params"][0] = new_p


@torch.no_grad()
def densify_and_prune(gaussians, densify_grad_threshold: float, clone_size_threshold: float,
                      prune_opacity_threshold: float, prune_size_threshold: float,
                      prune_screensize_threshold: Optional[float] = None, optimizer=None,
                      generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """Prune, clone and split in place on `gaussians`; returns preserve_idx (the kept row indices), as
    GaussianModel.densify_and_prune does.  With `optimizer` (torch.optim.Adam or GaussianAdam holding the
    reference's named groups) the Adam state is re-indexed in the same launch -- do not call the reference's
    update_optimizer_parameters afterwards then."""
    lib = _native.load()
    params = {k: getattr(gaussians, f"_{k}") for k in PARAMETER_NAMES}
    xyz = params["xyz"]
    dev = xyz.device
    if dev.type != "cuda":
        raise RuntimeError("densify_and_prune: the Gaussians must live on the GPU")
    N = int(xyz.shape[0])
    for k, t in params.items():
        if t.shape[0] != N or t.dtype != torch.float32 or not t.is_contiguous():
            raise RuntimeError(f"densify_and_prune: _{k} must be a contiguous fp32 (N, ...) tensor")
    scale = float(gaussians.spatial_scale)
    stats = {k: _f32(getattr(gaussians, k)) for k in _STATS}
    stream = _stream_handle(dev)

    apply_size = prune_screensize_threshold is not None
    args = _native.DensifyArgs(
        N, params["opacity"].data_ptr(), params["scaling"].data_ptr(), stats["max_radii2D"].data_ptr(),
        stats["xyz_grad_accum"].data_ptr(), stats["xyz_grad_count"].data_ptr(),
        float(prune_opacity_threshold), float(prune_screensize_threshold if apply_size else 0.0),
        float(prune_size_threshold) * scale, float(densify_grad_threshold), float(clone_size_threshold) * scale,
        int(apply_size and bool(getattr(gaussians, "use_screensize_threshold", True))), int(apply_size))
    ws = torch.empty(max(1, lib.gsr_densify_workspace_bytes(N)), dtype=torch.uint8, device=dev)
    counts = torch.empty(3, dtype=torch.int32, device=dev)
    preserve = torch.empty(max(N, 1), dtype=torch.int64, device=dev)
    _native.check(lib.gsr_densify_classify(args, ws.data_ptr(), counts.data_ptr(), preserve.data_ptr(), stream),
                  "gsr_densify_classify")
    n_keep, n_clone, n_split = (int(c) for c in counts.tolist())
    n_new = n_keep + n_clone + n_split
    z = torch.empty((n_split, 3), dtype=torch.float32, device=dev)
    if n_split:
        z.normal_(0.0, 1.0, generator=generator)

    _scatter_and_rebind(lib, gaussians, params, stats, optimizer, ws, z, N, n_new, stream)
    return preserve[:n_keep]


@torch.no_grad()
def prune_points(gaussians, keep_mask: torch.Tensor, optimizer=None) -> torch.Tensor:
    """Remove the rows where keep_mask (N,) bool is False, in place on `gaussians`; returns preserve_idx.  The rows move
    as densify_and_prune moves its kept rows -- parameters, Adam moments (with `optimizer`) and the three
    densification statistics in one scatter launch (gsr_densify_classify_keep + gsr_densify_apply)."""
    dev = gaussians._xyz.device
    N = int(gaussians._xyz.shape[0])
    if not torch.is_tensor(keep_mask) or tuple(keep_mask.shape) != (N,) or keep_mask.dtype != torch.bool:
        raise RuntimeError(f"prune_points: keep_mask must be a bool tensor of shape ({N},)")
    if dev.type != "cuda":
        raise RuntimeError("prune_points: the Gaussians must live on the GPU")
    lib = _native.load()
    params = {k: getattr(gaussians, f"_{k}") for k in PARAMETER_NAMES}
    for k, t in params.items():
        if t.shape[0] != N or t.dtype != torch.float32 or not t.is_contiguous():
            raise RuntimeError(f"prune_points: _{k} must be a contiguous fp32 (N, ...) tensor")
    keep = keep_mask.to(dev).contiguous()
    stats = {k: _f32(getattr(gaussians, k)) for k in _STATS}
    stream = _stream_handle(dev)
    ws = torch.empty(max(1, lib.gsr_densify_workspace_bytes(N)), dtype=torch.uint8, device=dev)
    counts = torch.empty(3, dtype=torch.int32, device=dev)
    preserve = torch.empty(max(N, 1), dtype=torch.int64, device=dev)
    _native.check(lib.gsr_densify_classify_keep(N, keep.data_ptr() if N else None, ws.data_ptr(), counts.data_ptr(),
                                                preserve.data_ptr(), stream), "gsr_densify_classify_keep")
    n_keep = int(counts[0].item())
    z = torch.empty((0, 3), dtype=torch.float32, device=dev)
    _scatter_and_rebind(lib, gaussians, params, stats, optimizer, ws, z, N, n_keep, stream)
    return preserve[:n_keep]


# ---- contribution statistics over a pass of views (rasterizer.contributions_raw) ----
_CONTRIB = dict(contrib_count=("count", torch.int64), contrib_wsum=("wsum", torch.float32),
                contrib_wmax=("wmax", torch.float32))


def _drop_contributions(gaussians) -> None:
    for k in _CONTRIB:
        if getattr(gaussians, k, None) is not None:
            setattr(gaussians, k, None)


def reset_contributions(gaussians) -> None:
    """Forget the accumulated contribution statistics (the next accumulate_contributions starts from zeros)."""
    _drop_contributions(gaussians)


@torch.no_grad()
def accumulate_contributions(gaussians, stats=None, rasterizer=None, **render_args) -> None:
    """Add one view's contribution statistics to gaussians.contrib_count (N,) int64, .contrib_wsum and .contrib_wmax
    (N,) float32 (count and wsum summed over the views, wmax their max), created as zeros by the first call after a
    reset or a change of the number of Gaussians.  Either `stats`, the dict of a contributions call on all N Gaussians
    (contributions_raw / GaussianRasterizer.contributions / rasterize_contributions), or `rasterizer`, a
    GaussianRasterizer whose contributions(**render_args) then accumulates straight into the buffers."""
    if (stats is None) == (rasterizer is None):
        raise RuntimeError("accumulate_contributions: give exactly one of stats and rasterizer")
    N = int(gaussians._xyz.shape[0])
    dev = gaussians._xyz.device
    if stats is not None:
        for attr, (name, dtype) in _CONTRIB.items():
            t = stats.get(name)
            if not torch.is_tensor(t) or tuple(t.shape) != (N,) or t.dtype != dtype:
                raise RuntimeError(f"accumulate_contributions: stats[{name!r}] must be a {dtype} tensor of shape ({N},)")
    for attr, (name, dtype) in _CONTRIB.items():
        cur = getattr(gaussians, attr, None)
        if cur is None or cur.shape[0] != N:
            setattr(gaussians, attr, torch.zeros(N, dtype=dtype, device=dev))
    if rasterizer is not None:
        out = {name: getattr(gaussians, attr) for attr, (name, _) in _CONTRIB.items()}
        rasterizer.contributions(out=out, accumulate=True, **render_args)
        return
    gaussians.contrib_count += stats["count"].to(dev)
    gaussians.contrib_wsum += stats["wsum"].to(dev)
    torch.maximum(gaussians.contrib_wmax, stats["wmax"].to(dev), out=gaussians.contrib_wmax)


@torch.no_grad()
def prune_by_contribution(gaussians, score="wmax", threshold: Optional[float] = None,
                          keep_ratio: Optional[float] = None, optimizer=None) -> torch.Tensor:
    """Prune by a per-Gaussian score: "wmax" (RadSplat), "wsum" (LightGaussian's significance without its volume
    term) or "count" of the accumulated statistics, or any (N,) tensor.  Exactly one of threshold (keep where
    score > threshold) and keep_ratio (keep the ceil(keep_ratio * N) highest; ties go to the lower index, through a
    stable sort).  Returns preserve_idx; the accumulated statistics are dropped (prune_points)."""
    if (threshold is None) == (keep_ratio is None):
        raise RuntimeError("prune_by_contribution: give exactly one of threshold and keep_ratio")
    N = int(gaussians._xyz.shape[0])
    if isinstance(score, str):
        if score not in ("wmax", "wsum", "count"):
            raise RuntimeError(f"prune_by_contribution: score must be 'wmax', 'wsum', 'count' or a tensor, got {score!r}")
        values = getattr(gaussians, f"contrib_{score}", None)
        if values is None or values.shape[0] != N:
            raise RuntimeError("prune_by_contribution: no accumulated statistics (accumulate_contributions first)")
    else:
        values = score
        if not torch.is_tensor(values) or tuple(values.shape) != (N,):
            raise RuntimeError(f"prune_by_contribution: a score tensor must have shape ({N},)")
    if threshold is not None:
        keep = values > threshold
    else:
        if not 0.0 <= float(keep_ratio) <= 1.0:
            raise RuntimeError("prune_by_contribution: keep_ratio must be in [0, 1]")
        import math
        n_keep = min(N, int(math.ceil(float(keep_ratio) * N)))
        order = torch.sort(values, descending=True, stable=True).indices
        keep = torch.zeros(N, dtype=torch.bool, device=values.device)
        keep[order[:n_keep]] = True
    return prune_points(gaussians, keep.to(gaussians._xyz.device), optimizer=optimizer)


# ---- 3DGS-MCMC (Kheradmand et al., NeurIPS 2024; gsplat's MCMCStrategy) on the kernels of csrc/gsr_mcmc.hip ----
# A training loop calls inject_noise after every optimizer step and, every refine interval, relocate_dead and then
# add_new.  MCMC's opacity and scale regularisers are two mean() calls in the loss and stay in torch.
_MCMC_KINDS = dict(opacity=_native.FIELD_OPACITY, scaling=_native.FIELD_SCALING)
_MULTINOMIAL_MAX = 2 ** 24  # torch.multinomial's limit on the number of categories


def _mcmc_params(gaussians, what: str):
    params = {k: getattr(gaussians, f"_{k}") for k in PARAMETER_NAMES}
    N = int(params["xyz"].shape[0])
    for k, t in params.items():
        if t.shape[0] != N or t.dtype != torch.float32 or not t.is_contiguous():
            raise RuntimeError(f"{what}: _{k} must be a contiguous fp32 (N, ...) tensor")
    for k, shape in (("xyz", (N, 3)), ("opacity", (N, 1)), ("scaling", (N, 3)), ("rotation", (N, 4))):
        if tuple(params[k].shape) != shape:
            raise RuntimeError(f"{what}: _{k} must have shape {shape}, got {tuple(params[k].shape)}")
    return params, N


def _need_gpu(params, what: str) -> None:
    """The last check before any launch: the arguments were valid, and there is no CPU path."""
    dev = params["xyz"].device
    if dev.type != "cuda" or any(t.device != dev for t in params.values()):
        raise RuntimeError(f"{what}: the Gaussians must live on the GPU")


def _check_min_opacity(min_opacity: float, what: str) -> float:
    if not 0.0 < float(min_opacity) < 1.0:
        raise RuntimeError(f"{what}: min_opacity must be in (0, 1)")
    return float(min_opacity)


def _draw_sources(probs: torch.Tensor, n: int, generator, multinomial_max: int = _MULTINOMIAL_MAX) -> torch.Tensor:
    """n indices into probs (M,), drawn with replacement with probability proportional to probs:
    torch.multinomial up to its 2^24 categories, the inverse of the cumulative sum (float64) above."""
    if probs.shape[0] <= multinomial_max:
        return torch.multinomial(probs, n, replacement=True, generator=generator)
    cdf = torch.cumsum(probs.double(), 0)
    u = torch.rand(n, dtype=torch.float64, device=probs.device, generator=generator) * cdf[-1]
    return torch.searchsorted(cdf, u, right=True).clamp_(max=probs.shape[0] - 1)


def _check_sampled(sampled_idx, n: int, N: int, dev, what: str) -> torch.Tensor:
    if not torch.is_tensor(sampled_idx) or tuple(sampled_idx.shape) != (n,) or sampled_idx.dtype != torch.int64:
        raise RuntimeError(f"{what}: sampled_idx must be an int64 tensor of shape ({n},)")
    if n and (int(sampled_idx.min()) < 0 or int(sampled_idx.max()) >= N):
        raise RuntimeError(f"{what}: sampled_idx out of range [0, {N})")
    return sampled_idx.to(dev).contiguous()


def _mcmc_fields(params, optimizer, n_out, in_place: bool):
    """The gsr_densify_field list of the six parameters (with their Adam moments when `optimizer` holds them), in
    place (dst = the tensors themselves) or into new tensors of n_out rows."""
    dev = params["xyz"].device
    fields, new_params, new_states, keep = [], {}, {}, []
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    for k in PARAMETER_NAMES:
        src = params[k]
        dst = src if in_place else torch.empty((n_out,) + tuple(src.shape[1:]), dtype=torch.float32, device=dev)
        new_params[k] = dst
        m_src = v_src = m_dst = v_dst = None
        if optimizer is not None:
            group = _group_for(optimizer, k, src)
            st = optimizer.state.get(group["params"][0], None) if group is not None else None
            if st is not None and "exp_avg" in st:
                m_src, v_src = st["exp_avg"], st["exp_avg_sq"]
                for t in (m_src, v_src):
                    if t.shape != src.shape or t.dtype != torch.float32 or t.device != dev:
                        raise RuntimeError(f"optimizer state of {k!r} does not match its parameter")
                if in_place:
                    if not (m_src.is_contiguous() and v_src.is_contiguous()):
                        raise RuntimeError(f"optimizer state of {k!r} must be contiguous")
                    m_dst, v_dst = m_src, v_src
                else:
                    m_src, v_src = m_src.contiguous(), v_src.contiguous()
                    m_dst, v_dst = torch.empty_like(dst), torch.empty_like(dst)
                new_states[k] = (group, st, m_dst, v_dst)
                keep += [m_src, v_src]
            elif group is not None:
                new_states[k] = (group, None, None, None)
        fields.append(_native.DensifyField(src.data_ptr(), dst.data_ptr(), ptr(m_src), ptr(v_src), ptr(m_dst),
                                           ptr(v_dst), src[0].numel(), _MCMC_KINDS.get(k, _native.FIELD_PLAIN)))
    return fields, new_params, new_states, keep


@torch.no_grad()
def mcmc_relocation(opacities: torch.Tensor, scales: torch.Tensor, ratios: torch.Tensor):
    """gsplat's compute_relocation: (new_opacities (n,), new_scales (n,3)) of activated opacities (n,) or (n,1), scales
    (n,3) and integer ratios (n,) (clamped to [1, 51]): o' = 1 - (1 - o)^(1/r), scales times
    c = o / sum_{k<r} C(r,k+1) (-1)^k o'^(k+1) / sqrt(k+1).  new_opacities has the shape of opacities."""
    n = int(scales.shape[0]) if torch.is_tensor(scales) and scales.dim() == 2 else -1
    if n < 0 or tuple(scales.shape) != (n, 3) or not torch.is_tensor(opacities) or opacities.numel() != n \
            or opacities.dim() not in (1, 2) or not torch.is_tensor(ratios) or tuple(ratios.shape) != (n,):
        raise RuntimeError("mcmc_relocation: opacities (n,) or (n,1), scales (n,3) and ratios (n,) are required")
    if opacities.dtype != torch.float32 or scales.dtype != torch.float32:
        raise RuntimeError("mcmc_relocation: opacities and scales must be float32")
    if ratios.dtype.is_floating_point or ratios.dtype == torch.bool:
        raise RuntimeError("mcmc_relocation: ratios must be an integer tensor")
    dev = scales.device
    if dev.type != "cuda" or opacities.device != dev or ratios.device != dev:
        raise RuntimeError("mcmc_relocation: the tensors must live on one GPU")
    lib = _native.load()
    o, s = opacities.detach().contiguous(), scales.detach().contiguous()
    r = ratios.clamp(1, _native.MCMC_MAX_RATIO).to(torch.int32).contiguous()
    new_o, new_s = torch.empty_like(o), torch.empty_like(s)
    if n:
        _native.check(lib.gsr_mcmc_relocation(n, o.data_ptr(), s.data_ptr(), 1, None, r.data_ptr(), n, 0.5,
                                              new_o.data_ptr(), new_s.data_ptr(), _stream_handle(dev)),
                      "gsr_mcmc_relocation")
    return new_o, new_s


@torch.no_grad()
def inject_noise(gaussians, scale: float, noise: Optional[torch.Tensor] = None,
                 generator: Optional[torch.Generator] = None) -> None:
    """gsplat's inject_noise_to_position in one launch, in place on gaussians._xyz:
    xyz += Sigma (z * gate * scale), Sigma = R(q) diag(exp(scaling)^2) R(q)^T, gate = sigmoid(100 ((1 - o) - 0.995)).
    scale: the xyz learning rate times the noise learning rate (gsplat: 5e5).  noise: the (N,3) standard normal draws
    z, drawn here with `generator` when not given."""
    params, N = _mcmc_params(gaussians, "inject_noise")
    dev = params["xyz"].device
    if noise is None:
        noise = torch.empty((N, 3), dtype=torch.float32, device=dev).normal_(0.0, 1.0, generator=generator)
    elif not torch.is_tensor(noise) or tuple(noise.shape) != (N, 3) or noise.dtype != torch.float32 \
            or noise.device != dev or not noise.is_contiguous():
        raise RuntimeError(f"inject_noise: noise must be a contiguous fp32 ({N}, 3) tensor on the parameters' device")
    _need_gpu(params, "inject_noise")
    if N == 0:
        return
    _native.check(_native.load().gsr_mcmc_noise(N, params["xyz"].data_ptr(), params["opacity"].data_ptr(),
                                                params["scaling"].data_ptr(), params["rotation"].data_ptr(),
                                                noise.data_ptr(), float(scale), _stream_handle(dev)), "gsr_mcmc_noise")


@torch.no_grad()
def relocate_dead(gaussians, min_opacity: float = 0.005, optimizer=None,
                  generator: Optional[torch.Generator] = None, sampled_idx: Optional[torch.Tensor] = None) -> int:
    """gsplat's relocate: every dead Gaussian (sigmoid(opacity) <= min_opacity) becomes a copy of an alive one drawn
    with probability proportional to its opacity; a source drawn k times gets the relocation values of ratio k + 1, and
    its Adam moments are zeroed (with `optimizer`).  In place: the parameter tensors, and so the optimizer's state keys,
    keep their identity.  sampled_idx (n_dead,) int64 pins the source rows (alive rows of [0, N)).  Returns the number
    of relocated rows; nothing is launched when no row is dead or none is alive."""
    params, N = _mcmc_params(gaussians, "relocate_dead")
    min_opacity = _check_min_opacity(min_opacity, "relocate_dead")
    dev = params["xyz"].device
    opac = torch.sigmoid(params["opacity"].detach()).reshape(-1)
    dead = opac <= min_opacity
    dead_idx = dead.nonzero().squeeze(-1)
    n = int(dead_idx.shape[0])
    if sampled_idx is not None:
        src = _check_sampled(sampled_idx, n, N, dev, "relocate_dead")
        if n and bool(dead[src].any()):
            raise RuntimeError("relocate_dead: sampled_idx names a dead row")
    _need_gpu(params, "relocate_dead")
    if n == 0 or n == N:
        return 0
    if sampled_idx is None:
        alive_idx = (~dead).nonzero().squeeze(-1)
        src = alive_idx[_draw_sources(opac[alive_idx], n, generator)]
    fields, _, _, keep = _mcmc_fields(params, optimizer, N, in_place=True)
    occ = torch.bincount(src, minlength=N).to(torch.int32)
    values = torch.empty((n, 4), dtype=torch.float32, device=dev)
    arr = (_native.DensifyField * len(fields))(*fields)
    _native.check(_native.load().gsr_mcmc_apply(N, n, src.data_ptr(), dead_idx.data_ptr(), occ.data_ptr(), min_opacity,
                                                values.data_ptr(), arr, len(fields), _stream_handle(dev)),
                  "gsr_mcmc_apply")
    return n


@torch.no_grad()
def add_new(gaussians, cap_max: int, growth: float = 1.05, min_opacity: float = 0.005, optimizer=None,
            generator: Optional[torch.Generator] = None, sampled_idx: Optional[torch.Tensor] = None) -> int:
    """gsplat's add_new: n_new = max(0, min(cap_max, int(growth * N)) - N) Gaussians are appended as copies of rows
    drawn from all rows with probability proportional to opacity; a source drawn k times (and its copies) gets the
    relocation values of ratio k + 1.  Parameters, statistics and (with `optimizer`) the Adam state are rebound as
    densify_and_prune rebinds them: old moments kept, new rows' moments and statistics zero; the contribution buffers
    are dropped.  sampled_idx (n_new,) int64 pins the source rows.  Returns n_new."""
    params, N = _mcmc_params(gaussians, "add_new")
    min_opacity = _check_min_opacity(min_opacity, "add_new")
    dev = params["xyz"].device
    n = max(0, min(int(cap_max), int(growth * N)) - N)
    if sampled_idx is not None:
        src = _check_sampled(sampled_idx, n, N, dev, "add_new")
    _need_gpu(params, "add_new")
    if n == 0:
        return 0
    if sampled_idx is None:
        src = _draw_sources(torch.sigmoid(params["opacity"].detach()).reshape(-1), n, generator)
    fields, new_params, new_states, keep = _mcmc_fields(params, optimizer, N + n, in_place=False)
    new_stats = {}
    for k in _STATS:
        old = _f32(getattr(gaussians, k))
        keep.append(old)
        new_stats[k] = torch.empty(N + n, dtype=torch.float32, device=dev)
        fields.append(_native.DensifyField(old.data_ptr(), new_stats[k].data_ptr(), None, None, None, None, 1,
                                           _native.FIELD_STAT))
    occ = torch.bincount(src, minlength=N).to(torch.int32)
    values = torch.empty((n, 4), dtype=torch.float32, device=dev)
    arr = (_native.DensifyField * len(fields))(*fields)
    _native.check(_native.load().gsr_mcmc_apply(N, n, src.data_ptr(), None, occ.data_ptr(), min_opacity,
                                                values.data_ptr(), arr, len(fields), _stream_handle(dev)),
                  "gsr_mcmc_apply")
    _drop_contributions(gaussians)
    _rebind(gaussians, optimizer, new_params, new_stats, new_states)
    return n
