"""Rendered alpha, a per-pixel background and the background's gradients (gsr_forward_ext / gsr_backward_ext) on the
GPU, against the CPU oracle and against the plain calls.

Base scene: 4000 Gaussians at 203x139 (13x9 tiles, both image edges partial tiles), SH degree 1, background
(0.3, 0.6, 0.9).  The oracle knows neither alpha nor a background image; the truth of every Gaussian gradient is
composed from it by linearity.  With upstream gradients (g, di, a) of (colour, inverse depth, alpha) and background B,
    L = sum g.(C + T_final B) + di.ID + a (1 - T_final)   =>   dL = [B = 0 terms] + tau dT_final,  tau = sum_c B_c g_c - a,
so the truth is the oracle's run A (background 0, SH colours, backward(g, di)) plus its run B (colours 0, background 1,
so colour channel 0 IS T_final; backward((tau, 0, 0))); dL/dshs is run A alone.  The composition's own error is
measured from the oracle alone on the vector background without alpha, where the oracle has a direct answer, recorded,
and added to the clean bar; no bar is fitted to HIP output.  Achieved figures: profiles/parity_alpha.json.  As in
tests/test_gpu_parity.py compare_backward, a second backward on the same forward with all three upstream gradients
zeroed on the oracle's flip candidates is held to that clean bar over ALL Gaussians, against truth - g_flip (the
composition is linear in (g, di, a)); figures in profiles/parity_masked.json.

Selections: those of tests/test_edge_parity.py plus the union walk and 32-instance segments.  The union walk is a form
of the whole-tile kernel, so its selection is the whole-tile one with bwd_union=1 (at this image size bwd_union alone
would leave the segmented walk in place)."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import parity
from tests.helpers import hip_state_arrays, rel_l2, run_hip, run_oracle, scene_inputs, settings_for, upstream
from tests.test_edge_parity import SELECTIONS as EDGE_SELECTIONS
from tests.test_gpu_parity import (COLOR_TOL, FLIP_MARGIN, FLIP_PIXEL_CAP, FLIP_PROPAGATION, FLIP_TOL, GRAD_CLEAN_TOL,
                                   GRADS, _case, compare_forward)

pytestmark = pytest.mark.gpu

N, W, H, SEED = 4000, 203, 139, 7
BG = (0.3, 0.6, 0.9)
SELECTIONS = dict(EDGE_SELECTIONS, union=dict(bwd_seg=0, bwd_parts=1, bwd_union=1), seg_k32=dict(seg_k=32))
GEOMETRY = ("means3D", "means2D", "opacities", "scales", "rotations")  # dL/dshs does not see T_final
CASES = ("alpha_vector_bg", "alpha_bg_image", "alpha_only")
f32 = np.float32


@functools.lru_cache(maxsize=None)
def _base():
    """(inputs, dL_dcolor, dL_dinvdepth, dL_dalpha, a random background image in [0, 1])."""
    inp = scene_inputs(N, W, H, sh_degree=1, seed=SEED, bg=BG)
    dc, di = upstream(W, H, SEED)
    rng = np.random.default_rng(SEED)
    return inp, dc, di, rng.standard_normal((1, H, W)).astype(f32), rng.random((3, H, W), dtype=f32)


@functools.lru_cache(maxsize=None)
def _oracle():
    """The oracle's forwards, run once: direct (the scene as it is), run A (background 0), run B (colours 0,
    background 1)."""
    inp = _base()[0]
    direct = run_oracle(inp)
    run_a = run_oracle(dict(inp, bg=np.zeros(3, f32)))[3]
    run_b = run_oracle(dict(inp, bg=np.ones(3, f32)), colors_precomp=np.zeros((N, 3), f32))[3]
    return direct, run_a, run_b


def _compose(g, di, tau):
    """Oracle run A's backward(g, di) plus run B's backward((tau, 0, 0)), in float64; shs from run A alone."""
    _, run_a, run_b = _oracle()
    t3 = np.zeros((3, H, W), f32)
    t3[0] = tau
    b = run_b.backward(t3, None)
    out = {k: b[k].astype(np.float64) for k in GEOMETRY}
    out["shs"] = np.zeros((N, 4, 3), np.float64)
    if g is not None:
        a = run_a.backward(g, di)
        for k in GRADS:
            out[k] = out[k] + a[k]
    return out


@functools.lru_cache(maxsize=None)
def _residual():
    """The composition against the oracle's direct vector-background backward (no alpha): relative L2 per gradient."""
    inp, dc, di, _, _ = _base()
    tau = np.einsum("c,chw->hw", np.asarray(BG, np.float64), dc.astype(np.float64)).astype(f32)
    comp, want = _compose(dc, di, tau), _oracle()[0][3].backward(dc, di)
    res = {k: rel_l2(comp[k], want[k]) for k in GRADS}
    parity.record("alpha_background_composition", "residual_vs_direct_oracle", res)
    return res


@functools.lru_cache(maxsize=None)
def _case_inputs(case):
    """(g, di, a, background) of one case and its composed truth, with the flip candidates' share g_flip and their
    mask."""
    inp, dc, di, da, image = _base()
    g, d = (None, None) if case == "alpha_only" else (dc, di)
    bg = image if case == "alpha_bg_image" else np.asarray(BG, f32)
    B = bg.astype(np.float64) if bg.ndim == 3 else np.asarray(BG, np.float64)[:, None, None]
    tau = -da[0].astype(np.float64)
    if g is not None:
        tau = tau + (B * g.astype(np.float64)).sum(0)
    tau = tau.astype(f32)
    flip = (_oracle()[0][3].threshold_margin() < FLIP_MARGIN).astype(f32)
    truth = _compose(g, d, tau)
    g_flip = _compose(None if g is None else g * flip[None], None if d is None else d * flip[None], tau * flip)
    return g, d, da, bg, truth, g_flip, flip.astype(bool)


def _t(a, dev):
    return None if a is None else torch.as_tensor(np.asarray(a, f32), device=dev)


def _forward(inp, dev, bg=None, return_alpha=True, colors=None):
    from gaussian_splatting_lightning_amd.rasterizer import forward_raw
    rs = settings_for(inp, dev)
    if bg is not None:
        rs = rs._replace(bg=_t(bg, dev))
    res = forward_raw(_t(inp["means3D"], dev), None if colors is not None else _t(inp["shs"], dev), _t(colors, dev),
                      _t(inp["opacities"], dev), _t(inp["scales"], dev), _t(inp["rotations"], dev), None, rs,
                      return_alpha=return_alpha)
    return rs, res


def _np(g):
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in g.items()}


def _same(a, b, keys=GRADS):
    for k in keys:
        assert torch.equal(a[k], b[k]), k


def test_scene_preconditions():
    """What the base scene must exercise, asserted from the oracle (no GPU work)."""
    direct, run_a, run_b = _oracle()
    run = direct[3]
    ft, nc = run.image_state()
    rg = run.ranges()
    flips = int((run.threshold_margin() < FLIP_MARGIN).sum())
    rec = dict(instances=int(run.num_rendered), longest_tile=int((rg[:, 1] - rg[:, 0]).max()),
               saturated=int((ft < 1e-3).sum()), above_half=int((ft > 0.5).sum()), untouched=int((nc == 0).sum()),
               flip_candidates=flips, pixels=W * H)
    parity.record("alpha_background_scene", "oracle_census", rec)
    assert rec["longest_tile"] > 64 and rec["saturated"] >= 1000 and rec["above_half"] >= 1000, rec
    assert rec["untouched"] >= 1 and flips <= 1e-3 * W * H, rec
    assert np.all(ft[nc == 0] == 1.0)
    # the three runs share their geometry: bit-equal transmittance, so run B's colour channel 0 is run A's T_final
    for other in (run_a, run_b):
        assert np.array_equal(other.image_state()[0].view(np.uint32), ft.view(np.uint32))


def test_alpha_is_one_minus_final_T(gpu_device):
    inp = _base()[0]
    direct = _oracle()[0]
    _, (color, radii, invd, alpha, st) = _forward(inp, gpu_device)
    assert alpha.shape == (1, H, W) and alpha.dtype == torch.float32
    hs = hip_state_arrays(dict(state=st, color=color.cpu().numpy(), radii=radii.cpu().numpy()))
    a = alpha[0].cpu().numpy()
    assert np.array_equal(a.view(np.uint32), (f32(1.0) - hs["final_T"]).view(np.uint32))
    # the two-render workaround this replaces: black Gaussians over a white background
    _, (white, _, _, _) = _forward(inp, gpu_device, bg=np.ones(3, f32), return_alpha=False, colors=np.zeros((N, 3), f32))
    assert np.array_equal(a.view(np.uint32), (f32(1.0) - white[0].cpu().numpy()).view(np.uint32))
    # against the oracle's transmittance
    ft, nc = direct[3].image_state()
    clean = direct[3].threshold_margin() >= FLIP_MARGIN
    err = np.abs(a - (f32(1.0) - ft))
    rec = dict(alpha_maxabs_clean=float(err[clean].max()), alpha_maxabs_all=float(err.max()),
               untouched_alpha_nonzero=int(np.count_nonzero(a[nc == 0])))
    parity.record(_case(), "alpha", rec)
    assert rec["alpha_maxabs_clean"] <= COLOR_TOL and rec["alpha_maxabs_all"] <= FLIP_TOL, rec
    assert rec["untouched_alpha_nonzero"] == 0
    # the other outputs are those of the plain call
    _, (c0, r0, i0, _) = _forward(inp, gpu_device, return_alpha=False)
    assert torch.equal(color, c0) and torch.equal(radii, r0) and torch.equal(invd, i0)


@pytest.mark.parametrize("knobs", [dict(fwd_parts=1), dict(fwd_parts=1, smask=0), dict(fwd_parts=2),
                                   dict(fwd_parts=4, bwd_seg=0), dict(fwd_parts=1, guard=1), dict(fwd_parts=2, guard=1),
                                   dict(fwd_parts=1, smask=0, guard=1), dict(fwd_parts=4, bwd_seg=0, guard=1),
                                   dict(fwd_parts=1, smask=0, fwd_whole_waves=6),
                                   dict(fwd_parts=1, smask=0, fwd_whole_waves=4), dict(fwd_parts=2, fwd_part_waves=4),
                                   dict(fwd_parts=4, bwd_seg=0, fwd_part_waves=4)],
                         ids=lambda k: "-".join(f"{n}{v}" for n, v in k.items()))
def test_every_forward_form_writes_alpha_and_the_image(gpu_device, knobs):
    """At 13x9 tiles the forward runs as 4 part-waves with checkpoints; the whole-tile forms (with and without strip
    masks), the 2-part form, the 4-part form without checkpoints and the guard's forms have the same epilogue, reached
    here by the knobs.  Under each: alpha is bitwise 1 - final_T of that render, a constant background image gives the
    vector call's bits, and (the guard apart, which decides threshold pixels by its own rule) alpha and the colour over
    a random image are bitwise the default form's."""
    from gaussian_splatting_lightning_amd import _native
    inp, _, _, _, image = _base()
    dev = gpu_device
    const = np.broadcast_to(np.asarray(BG, f32)[:, None, None], (3, H, W)).copy()
    _, (c_def, _, _, a_def, _) = _forward(inp, dev, bg=image)
    with _native.tuned(**knobs):
        _, (c_v, r_v, i_v, a_v, st_v) = _forward(inp, dev)
        _, (c_c, _, i_c, a_c, _) = _forward(inp, dev, bg=const)
        _, (c_i, _, _, a_i, _) = _forward(inp, dev, bg=image)
        _, (c_p, _, i_p, _) = _forward(inp, dev, return_alpha=False)
    final_T = hip_state_arrays(dict(state=st_v, color=c_v.cpu().numpy(), radii=r_v.cpu().numpy()))["final_T"]
    assert np.array_equal(a_v[0].cpu().numpy().view(np.uint32), (f32(1.0) - final_T).view(np.uint32))
    assert torch.equal(c_c, c_v) and torch.equal(a_c, a_v) and torch.equal(i_c, i_v)
    assert torch.equal(c_p, c_v) and torch.equal(i_p, i_v) and torch.equal(a_i, a_v)
    if "guard" not in knobs:
        assert torch.equal(a_i, a_def) and torch.equal(c_i, c_def)
    else:
        assert float((c_i - c_def).abs().max()) <= FLIP_TOL and float((a_i - a_def).abs().max()) <= FLIP_TOL


@pytest.mark.parametrize("selection", list(SELECTIONS))
@pytest.mark.parametrize("case", CASES)
def test_gradients_vs_composed_oracle(gpu_device, case, selection):
    from gaussian_splatting_lightning_amd import _native
    from gaussian_splatting_lightning_amd.rasterizer import backward_raw
    inp = _base()[0]
    g, d, da, bg, truth, g_flip, flip = _case_inputs(case)
    residual = _residual()
    with _native.tuned(**SELECTIONS[selection]):
        # the flip census of this selection's own forward (compare_forward: integer state, colour, touched Gaussians)
        run = compare_forward(inp, run_hip(inp, gpu_device), _oracle()[0])
        rs, (_, _, _, _, st) = _forward(inp, gpu_device, bg=bg)
        got = _np(backward_raw(st, rs, _t(g, gpu_device), _t(d, gpu_device), grad_out_alpha=_t(da, gpu_device)))
        got_m = None
        if flip.any():  # the masked leg (compare_backward): every upstream gradient zeroed on the flip candidates
            keep = (~flip).astype(f32)[None]
            got_m = _np(backward_raw(st, rs, _t(None if g is None else g * keep, gpu_device),
                                     _t(None if d is None else d * keep, gpu_device),
                                     grad_out_alpha=_t(da * keep, gpu_device)))
    clean = ~run.flip_touched
    rec = {"touched_gaussians": int(run.flip_touched.sum()), "flip_pixels": int(run.flip_mask.sum()),
           "flip_pixel_share": float(flip.mean())}
    for k in GRADS:
        want = truth[k].reshape(got[k].shape)
        norm = float(np.linalg.norm(want))
        rec[k] = dict(rel_l2=rel_l2(got[k], want), rel_l2_clean=rel_l2(got[k][clean], want[clean]),
                      bar=GRAD_CLEAN_TOL + FLIP_PROPAGATION * float(np.linalg.norm(g_flip[k])) / max(norm, 1e-30),
                      bar_clean=GRAD_CLEAN_TOL + residual[k])
        if got_m is not None:  # the composed truth is linear in (g, d, da): masked truth = truth - g_flip
            want_m = (truth[k] - g_flip[k]).reshape(got[k].shape)
            rec[k].update(rel_l2_masked=rel_l2(got_m[k], want_m),
                          rel_l2_masked_touched=rel_l2(got_m[k][~clean], want_m[~clean]))
    parity.record(_case(), "backward", rec)
    assert rec["flip_pixel_share"] <= FLIP_PIXEL_CAP, rec
    for k in GRADS:
        assert rec[k]["rel_l2_clean"] <= rec[k]["bar_clean"], (k, rec[k])
        assert rec[k]["rel_l2"] <= rec[k]["bar"], (k, rec[k])
        if got_m is not None:  # all Gaussians, the touched ones included, at the clean bar
            assert rec[k]["rel_l2_masked"] <= rec[k]["bar_clean"], (k, rec[k])


def test_background_image(gpu_device):
    from gaussian_splatting_lightning_amd.rasterizer import backward_raw
    inp, dc, di, da, image = _base()
    dev = gpu_device
    up = (_t(dc, dev), _t(di, dev))
    # a constant image is the vector call, bit for bit
    rs_v, (c_v, r_v, i_v, a_v, st_v) = _forward(inp, dev)
    const = np.broadcast_to(np.asarray(BG, f32)[:, None, None], (3, H, W)).copy()
    rs_c, (c_c, r_c, i_c, a_c, st_c) = _forward(inp, dev, bg=const)
    assert torch.equal(c_c, c_v) and torch.equal(r_c, r_v) and torch.equal(i_c, i_v) and torch.equal(a_c, a_v)
    g_v = backward_raw(st_v, rs_v, *up, grad_out_alpha=_t(da, dev), background_grad=True)
    g_c = backward_raw(st_c, rs_c, *up, grad_out_alpha=_t(da, dev), background_grad=True)
    _same(g_c, g_v)
    assert g_v["bg"].shape == (3,) and g_c["bg"].shape == (3, H, W)
    # a random image: C + final_T B, formed in torch from the background-0 render
    _, (c_0, _, _, _) = _forward(inp, dev, bg=np.zeros(3, f32), return_alpha=False)
    _, (c_i, _, _, a_i, st_i) = _forward(inp, dev, bg=image)
    final_T = torch.as_tensor(hip_state_arrays(dict(state=st_i, color=c_i.cpu().numpy(), radii=r_v.cpu().numpy()))["final_T"],
                              device=dev)
    err = float((c_i - (c_0 + final_T[None] * _t(image, dev))).abs().max())
    parity.record(_case(), "color_vs_composed", dict(maxabs=err))
    assert err <= COLOR_TOL, err
    assert torch.equal(a_i, a_v)
    with pytest.raises(RuntimeError):
        _forward(inp, dev, bg=np.zeros((3, H, W + 1), f32))
    with pytest.raises(RuntimeError):
        _forward(inp, dev, bg=np.zeros((1, 3), f32))


def test_background_gradients(gpu_device):
    from gaussian_splatting_lightning_amd.rasterizer import backward_chunked, backward_raw
    inp, dc, di, da, image = _base()
    dev = gpu_device
    up = (_t(dc, dev), _t(di, dev))
    rs_i, (c_i, r_i, _, _, st_i) = _forward(inp, dev, bg=image)
    final_T = hip_state_arrays(dict(state=st_i, color=c_i.cpu().numpy(), radii=r_i.cpu().numpy()))["final_T"]
    g_i = backward_raw(st_i, rs_i, *up, background_grad=True)
    assert np.array_equal(g_i["bg"].cpu().numpy().view(np.uint32), (final_T[None] * dc).view(np.uint32))
    # the 3-vector: a fixed float32 tree over the pixels, within a pairwise tree's bound of the float64 sum
    rs_v, (_, _, _, _, st_v) = _forward(inp, dev)
    g_v = backward_raw(st_v, rs_v, *up, background_grad=True)
    prod = final_T[None].astype(np.float64) * dc.astype(np.float64)
    want, bound = prod.sum((1, 2)), 4.0 * math.log2(W * H) * 2.0 ** -24 * np.abs(prod).sum((1, 2))
    got = g_v["bg"].cpu().numpy().astype(np.float64)
    parity.record(_case(), "vector_gradient", dict(err=np.abs(got - want).tolist(), bound=bound.tolist()))
    assert np.all(np.abs(got - want) <= bound), (got, want, bound)
    # the same bits on a second call, into a caller's destination, and from the compositing stage alone
    dst = torch.full((3,), float("nan"), device=dev)
    again = backward_raw(st_v, rs_v, *up, out={"bg": dst})
    assert again["bg"] is dst and torch.equal(dst, g_v["bg"])
    staged = torch.full((3,), float("nan"), device=dev)
    backward_chunked(st_v, rs_v, *up, chunks=[], bg_out=staged)
    assert torch.equal(staged, g_v["bg"])
    staged_i = torch.full((3, H, W), float("nan"), device=dev)
    backward_chunked(st_i, rs_i, *up, chunks=[], bg_out=staged_i)
    assert torch.equal(staged_i, g_i["bg"])
    # the background's gradient does not depend on alpha's, and asking for it moves nothing else
    _same(backward_raw(st_v, rs_v, *up), g_v)
    assert torch.equal(backward_raw(st_v, rs_v, *up, grad_out_alpha=_t(da, dev), background_grad=True)["bg"], g_v["bg"])


@pytest.mark.parametrize("image", [False, True])
def test_autograd(gpu_device, image):
    from gaussian_splatting_lightning_amd import GaussianRasterizer
    from gaussian_splatting_lightning_amd.rasterizer import backward_raw
    inp, dc, di, da, bgimg = _base()
    dev = gpu_device
    names = ("means3D", "opacities", "scales", "rotations", "shs")

    def leaves():
        p = {k: _t(inp[k], dev).requires_grad_(True) for k in names}
        p["means2D"] = torch.zeros_like(p["means3D"], requires_grad=True)
        p["bg"] = _t(bgimg if image else np.asarray(BG, f32), dev).requires_grad_(True)
        return p

    def render(p):
        r = GaussianRasterizer(settings_for(inp, dev)._replace(bg=p["bg"]), return_alpha=True)
        return r(means3D=p["means3D"], means2D=p["means2D"], shs=p["shs"], colors_precomp=None,
                 opacities=p["opacities"], scales=p["scales"], rotations=p["rotations"], cov3D_precomp=None)

    rs, (_, _, _, alpha_raw, st) = _forward(inp, dev, bg=bgimg if image else None)
    p = leaves()
    color, radii, invd, alpha = render(p)
    assert alpha.shape == (1, H, W) and alpha.requires_grad and torch.equal(alpha, alpha_raw)
    ((color * _t(dc, dev)).sum() + (alpha * _t(da, dev)).sum()).backward()
    want = backward_raw(st, rs, _t(dc, dev), None, grad_out_alpha=_t(da, dev), background_grad=True)
    for k in names + ("means2D", "bg"):
        assert p[k].grad is not None and p[k].grad.shape == p[k].shape, k
        assert torch.equal(p[k].grad, want[k].reshape(p[k].shape)), k
    # an alpha-only loss
    p = leaves()
    (render(p)[3] * _t(da, dev)).sum().backward()
    want = backward_raw(st, rs, None, None, grad_out_alpha=_t(da, dev), background_grad=True)
    for k in names + ("means2D", "bg"):
        assert torch.equal(p[k].grad, want[k].reshape(p[k].shape)), k
    assert not p["bg"].grad.any() and p["opacities"].grad.any()
    # without return_alpha the call returns its three outputs, and bg still receives its gradient
    p = leaves()
    out = GaussianRasterizer(settings_for(inp, dev)._replace(bg=p["bg"]))(
        means3D=p["means3D"], means2D=p["means2D"], shs=p["shs"], colors_precomp=None, opacities=p["opacities"],
        scales=p["scales"], rotations=p["rotations"], cov3D_precomp=None)
    assert len(out) == 3
    (out[0] * _t(dc, dev)).sum().backward()
    assert torch.equal(p["bg"].grad, backward_raw(st, rs, _t(dc, dev), None, background_grad=True)["bg"])


def test_unused_ext_is_neutral(gpu_device, monkeypatch):
    """The default call never reaches the ext entry points, and the ext path with nothing to add (alpha returned, a
    zero alpha gradient) gives the plain call's bits."""
    from gaussian_splatting_lightning_amd import _native
    from gaussian_splatting_lightning_amd.rasterizer import backward_raw
    inp, dc, di, _, _ = _base()
    dev = gpu_device
    up = (_t(dc, dev), _t(di, dev))
    lib = _native.load()

    def unreachable(*_a):
        raise AssertionError("the plain call went through an ext entry point")

    with monkeypatch.context() as m:
        m.setattr(lib, "gsr_forward_ext", unreachable)
        m.setattr(lib, "gsr_backward_ext", unreachable)
        rs, (c0, r0, i0, st0) = _forward(inp, dev, return_alpha=False)
        g0 = backward_raw(st0, rs, *up)
        assert "bg" not in g0
    _, (c1, r1, i1, _, st1) = _forward(inp, dev)
    assert torch.equal(c1, c0) and torch.equal(r1, r0) and torch.equal(i1, i0)
    _same(backward_raw(st1, rs, *up, grad_out_alpha=torch.zeros(1, H, W, device=dev)), g0)
    _same(backward_raw(st1, rs, *up, background_grad=True), g0)


@pytest.mark.parametrize("scene", ["no_gaussians", "all_behind_camera"])
def test_empty_scenes(gpu_device, scene):
    from gaussian_splatting_lightning_amd.rasterizer import backward_raw
    w, h = 40, 24
    dev = gpu_device
    inp = scene_inputs(300, w, h, sh_degree=0, seed=1, bg=(0.25, 0.5, 0.75))
    if scene == "no_gaussians":
        inp = {k: (v[:0] if k in ("means3D", "opacities", "scales", "rotations", "shs") else v) for k, v in inp.items()}
    else:
        inp["means3D"] = inp["means3D"] - np.array([0, 0, 50.0], f32) @ np.linalg.inv(inp["viewmatrix"][:3, :3])
    rng = np.random.default_rng(3)
    image, dc = rng.random((3, h, w), dtype=f32), rng.standard_normal((3, h, w)).astype(f32)
    da = _t(rng.standard_normal((1, h, w)), dev)
    for bg in (image, np.asarray(inp["bg"], f32)):
        rs, (color, radii, invd, alpha, st) = _forward(inp, dev, bg=bg)
        assert st.num_rendered == 0 and not radii.any() and not alpha.any() and not invd.any()
        assert torch.equal(color, _t(bg, dev) if bg.ndim == 3 else _t(bg, dev)[:, None, None].expand(3, h, w))
        g = backward_raw(st, rs, _t(dc, dev), None, grad_out_alpha=da, background_grad=True)
        if bg.ndim == 3:
            assert torch.equal(g["bg"], _t(dc, dev))  # T_final = 1
        else:
            want = dc.astype(np.float64).sum((1, 2))
            bound = 4.0 * math.log2(w * h) * 2.0 ** -24 * np.abs(dc).astype(np.float64).sum((1, 2))
            assert np.all(np.abs(g["bg"].cpu().numpy() - want) <= bound)
        for k in GRADS:
            assert g[k] is None or not g[k].any(), k


def test_chunked_backward_with_alpha(gpu_device):
    from gaussian_splatting_lightning_amd.rasterizer import backward_chunked, backward_raw
    inp, dc, di, da, image = _base()
    dev = gpu_device
    widths = dict(means3D=3, scales=3, rotations=4, opacities=1, means2D=3, shs=12)
    for bg in (None, image):
        rs, (_, _, _, _, st) = _forward(inp, dev, bg=bg)
        ref = backward_raw(st, rs, _t(dc, dev), _t(di, dev), grad_out_alpha=_t(da, dev))
        chunks = [(g0, g1, {k: torch.full((g1 - g0, w), float("nan"), device=dev) for k, w in widths.items()})
                  for g0, g1 in ((0, 1500), (1500, N))]
        backward_chunked(st, rs, _t(dc, dev), _t(di, dev), chunks, grad_out_alpha=_t(da, dev))
        for k in widths:
            assert torch.equal(torch.cat([o[k] for _, _, o in chunks], 0), ref[k].reshape(N, -1)), k
