"""The median depth map (gsr_forward_median / gsr_backward_median, forward_raw(median_depth=True),
backward_raw(grad_out_median_depth=...), rasterize_gaussians(median_depth=True)) and the normal consistency on the
blended surface (normal_consistency(median_depth=, depth_ratio=)) on the GPU.

Truth: tests/median_cases.py through tests/golden/median.npz -- the CPU oracle alone: each pixel's contributors front to
back with the oracle's weights, the incoming transmittance 1 - sum_(j<i) w_j in float64, the median the last contributor
with that above 0.5, its depth the oracle's.  A pixel with an incoming transmittance within the scene's MEDIAN_MARGIN
of 0.5 is a candidate (at most 0.1 % of a scene's pixels, asserted): there the device may select either of the two
contributors adjacent to the crossing; every other pixel is compared in full, the depth bit for bit.

Bars of the gradients (median_cases.bar): the larger of the suite's clean bar (GRAD_CLEAN_TOL) and 4 x the error of a
numpy float32 restatement, which sums the same pixels in another order, against the float64 truth -- computed by the
generator and stored in the fixture, never taken from the device.  The surface normals are held to the bars of
tests/test_normals.py: 4 x the float32 torch restatement's own error against float64 on the same input, at least four
fp32 roundings.  Achieved figures: profiles/parity_median.json.
"""
import numpy as np
import pytest
import torch

from tests import absgrad_cases as AC
from tests import feature_cases as F
from tests import median_cases as MC
from tests import normal_cases as NC
from tests import parity
from tests import test_alpha_background as TAB
from tests.helpers import rel_l2, run_oracle, settings_for
from tests.test_gpu_parity import GRAD_CLEAN_TOL, GRAD_TOL_ADHOC

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
CAMERA_TOL = 2e-5  # the camera-gradient bar of tests/test_distortion.py
FORWARD_FORMS = next(m for m in TAB.test_every_forward_form_writes_alpha_and_the_image.pytestmark
                     if m.name == "parametrize").args[1]
GEOMETRY = ("means3D", "means2D", "opacities", "scales", "rotations")
UNTOUCHED = ("means2D", "opacities", "scales", "rotations", "shs")  # what the median's gradient never reaches
CAMERA = ("viewmatrix", "projmatrix", "campos")
LAST_SELECTED = dict(A=218, A2=16, B=51)  # pixels whose median is their last contributor, by the oracle
C_FEAT = 7


def _t(a, dev):
    return None if a is None else torch.as_tensor(np.asarray(a, f32), device=dev)


def _forward(inp, dev, median=True, return_alpha=False, **kw):
    """forward_raw on the scene with SH colours.  Returns (settings, result tuple)."""
    from gaussian_splatting_lightning_amd.rasterizer import forward_raw
    rs = settings_for(inp, dev)
    if "features" in kw:
        kw["features"] = _t(kw["features"], dev)
    if median:
        kw["median_depth"] = True
    res = forward_raw(_t(inp["means3D"], dev), _t(inp["shs"], dev), None, _t(inp["opacities"], dev),
                      _t(inp["scales"], dev), _t(inp["rotations"], dev), None, rs, return_alpha=return_alpha, **kw)
    return rs, res


def _run(inp, dev, median=True, dc=None, di=None, gM=None, fwd=None, **kw):
    """Forward + backward_raw; returns (gradients on the device, (median_depth, median_index) or None)."""
    from gaussian_splatting_lightning_amd.rasterizer import backward_raw
    rs, res = _forward(inp, dev, median, **(fwd or {}))
    if gM is not None:
        kw["grad_out_median_depth"] = _t(gM, dev)
    g = backward_raw(res[-1], rs, _t(dc, dev), _t(di, dev), **kw)
    torch.cuda.synchronize()
    return g, ((res[-3], res[-2]) if median else None)


def _bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32),
                                                                     b.contiguous().view(torch.int32))


def _truth(name):
    t = MC.fixture_truth(name)
    assert int(t["flip_candidates"]) == 0
    assert int(t["candidate"].sum()) <= MC.MAX_CANDIDATE_FRACTION * t["candidate"].size
    return t


# ------------------------------------------------------------------------------------------------ 1. forward parity
@pytest.mark.parametrize("name", MC.SCENES)
def test_forward_parity(gpu_device, name):
    inp = MC.scene(name)
    t = _truth(name)
    n, W, H = AC.SCENES[name][:3]
    _, (color, radii, invd, alpha, md, mi, st) = _forward(inp, gpu_device, return_alpha=True)
    assert md.shape == (1, H, W) and md.dtype == torch.float32 and mi.shape == (1, H, W) and mi.dtype == torch.int32
    assert st.median.pos.shape == (H, W) and st.median.pos.dtype == torch.int32
    index, depth = mi[0].cpu().numpy(), md[0].cpu().numpy()
    cand = t["candidate"]
    rec = dict(pixels=int(W * H), candidates=int(cand.sum()), margin=float(t["margin"]), closest=float(t["closest"]),
               index_mismatches=int((index != t["index"])[~cand].sum()),
               depth_bit_mismatches=int((depth.view(np.uint32) != t["depth"].view(np.uint32))[~cand].sum()),
               candidates_off_the_crossing=int((~(index[..., None] == t["adjacent"]).any(-1))[cand].sum()),
               candidates_on_the_truth=int((index == t["index"])[cand].sum()),
               last_selected=int(t["last"].sum()), untouched=int((t["index"] < 0).sum()))
    parity.record(f"median_forward_{name}", "maps_vs_oracle", rec)
    print(name, rec)
    assert rec["index_mismatches"] == 0 and rec["depth_bit_mismatches"] == 0, rec  # every non-candidate pixel
    assert rec["candidates_off_the_crossing"] == 0, rec
    # a candidate's depth is that of the Gaussian it selected
    assert np.array_equal(depth[cand].view(np.uint32), t["z"][index[cand]].view(np.uint32))
    # exactly 0 and -1 where no Gaussian reaches (alpha is exactly 0 there): 12 pixels of scene A
    untouched = (alpha[0] == 0).cpu().numpy()
    assert int(untouched.sum()) == (12 if name == "A" else 0)
    assert np.all(depth[untouched] == 0) and np.all(index[untouched] == -1) and np.all(index[~untouched] >= 0)
    assert torch.all(st.median.pos[torch.as_tensor(untouched)] == -1)
    # pixels that never fall to half transparency before their last contributor select it
    assert rec["last_selected"] == LAST_SELECTED[name]
    assert np.array_equal(index[t["last"] & ~cand], t["index"][t["last"] & ~cand])
    # colour, radii, inverse depth and alpha are those of the call without the median
    _, (c0, r0, i0, a0, _) = _forward(inp, gpu_device, median=False, return_alpha=True)
    assert _bits(color, c0) and torch.equal(radii, r0) and _bits(invd, i0) and _bits(alpha, a0)


# ------------------------------------------------------------------------------------------------ 2. forward forms
@pytest.mark.parametrize("knobs", list(FORWARD_FORMS) + [dict(guard=1)],
                         ids=lambda k: "-".join(f"{n}{v}" for n, v in k.items()))
def test_every_forward_form_gives_the_same_maps(gpu_device, knobs):
    from gaussian_splatting_lightning_amd import _native
    for name in ("A", "B"):
        inp = MC.scene(name)
        _truth(name)  # (no alpha-threshold flip candidate: the guarded decision is the plain one on every pair)
        want = _forward(inp, gpu_device)[1]
        with _native.tuned(**knobs):
            got = _forward(inp, gpu_device)[1]
        assert _bits(got[-3], want[-3]) and _bits(got[-2], want[-2]), name  # the replay reads only recorded state


# ------------------------------------------------------------------------------------------------ 3. backward alone
def _compare(case, got, truth, t, names):
    rec = {}
    for k in names:
        norm = float(np.linalg.norm(truth[k]))
        bar = MC.bar(t, k, GRAD_CLEAN_TOL, norm) if k == "means3D" else GRAD_CLEAN_TOL
        rec[k] = dict(rel_l2=rel_l2(got[k].cpu().numpy().reshape(np.shape(truth[k])), truth[k]), bar=bar)
    parity.record(case, "backward", rec)
    print(case, {k: (v["rel_l2"], v["bar"]) for k, v in rec.items()})
    for k in names:
        assert rec[k]["rel_l2"] <= rec[k]["bar"], (case, k, rec[k])


@pytest.mark.parametrize("knobs", [{}, dict(bwd_live=0), dict(bwd_prezero=0)],
                         ids=lambda k: "-".join(f"{n}{v}" for n, v in k.items()) or "default")
@pytest.mark.parametrize("name", MC.SCENES)
def test_backward_parity_median_alone(gpu_device, name, knobs):
    """Every gradient comes from the median depth (the colour's upstream gradient is absent): the live-flag case."""
    from gaussian_splatting_lightning_amd import _native
    inp = MC.scene(name)
    t = _truth(name)
    n = AC.SCENES[name][0]
    with _native.tuned(**knobs):
        g, _ = _run(inp, gpu_device, gM=MC.upstream(name), camera_grads=True)
    _compare(f"median_alone_{name}_" + ("-".join(f"{k}{v}" for k, v in knobs.items()) or "default"), g, t, t,
             ("means3D",))
    # the Gaussians with a gradient are exactly the truth's: none dropped by the live flags, none invented
    got_nz = (g["means3D"] != 0).any(1).cpu().numpy()
    assert np.array_equal(got_nz, t["dz"] != 0), (int(got_nz.sum()), int((t["dz"] != 0).sum()))
    for k in UNTOUCHED:
        assert float(g[k].abs().max()) == 0.0, k
    # the camera: z = [p, 1] . V[:, 2], so dL/dV[:, 2] = sum_i dz_i [p_i, 1]
    want = MC.camera_column(name, t["dz"])
    rec = dict(rel_l2=rel_l2(g["viewmatrix"][:, 2].cpu().numpy(), want), bar=CAMERA_TOL)
    parity.record(f"median_camera_{name}", "viewmatrix_column_2", rec)
    print(name, rec)
    assert rec["rel_l2"] <= CAMERA_TOL and float(np.abs(want).max()) > 0, rec


# ------------------------------------------------------------------------------------------------ 4. joint call
@pytest.mark.parametrize("name", MC.SCENES)
def test_backward_parity_joint_with_colour(gpu_device, name):
    """SH colour + inverse depth + median depth in one call."""
    inp, dc, di = F.scene(name)
    t = _truth(name)
    run = run_oracle(dict(inp, bg=np.zeros(3, f32)))[3]
    assert int((run.threshold_margin() < AC.FLIP_MARGIN).sum()) == 0
    a = run.backward(dc, di)
    truth = {k: a[k].astype(f64) for k in GEOMETRY + ("shs",)}
    truth["means3D"] = truth["means3D"] + t["means3D"]
    g, _ = _run(inp, gpu_device, dc=dc, di=di, gM=MC.upstream(name))
    _compare(f"median_joint_{name}", g, truth, t, GEOMETRY + ("shs",))


@pytest.mark.parametrize("name", ["A", "B"])
def test_no_median_gradient_keeps_every_bit(gpu_device, name):
    from tests import distortion_cases as DC
    inp, dc, di = F.scene(name)
    plain, _ = _run(inp, gpu_device, False, dc, di, camera_grads=True)
    g, _ = _run(inp, gpu_device, True, dc, di, None, camera_grads=True)
    for k in GEOMETRY + ("shs",) + CAMERA:
        assert _bits(g[k], plain[k]), k
    # together with features and the distortion map
    f, dF = F.inputs(name, C_FEAT)
    both = dict(features=f, distortion="ndc", distortion_near=DC.NEAR, distortion_far=DC.FAR)
    kw = dict(grad_out_features=_t(dF, gpu_device), grad_out_distortion=_t(DC.upstream(name), gpu_device),
              camera_grads=True)
    plain, _ = _run(inp, gpu_device, False, dc, di, fwd=both, **kw)
    g, _ = _run(inp, gpu_device, True, dc, di, None, fwd=both, **kw)
    for k in GEOMETRY + ("shs", "features") + CAMERA:
        assert _bits(g[k], plain[k]), k
    # and with its gradient the median adds to means3D alone
    g, _ = _run(inp, gpu_device, True, dc, di, MC.upstream(name), fwd=both, **kw)
    for k in UNTOUCHED + ("features",):
        assert _bits(g[k], plain[k]), k
    assert not _bits(g["means3D"], plain["means3D"])


# ------------------------------------------------------------------------------------------------ 5. determinism
@pytest.mark.parametrize("name", MC.SCENES)
def test_calls_repeat_bit_for_bit(gpu_device, name):
    from gaussian_splatting_lightning_amd.rasterizer import backward_raw, contributions_raw
    inp, dc, di = F.scene(name)
    gM = MC.upstream(name)
    a, Ma = _run(inp, gpu_device, dc=dc, di=di, gM=gM, camera_grads=True)
    b, Mb = _run(inp, gpu_device, dc=dc, di=di, gM=gM, camera_grads=True)
    assert _bits(Ma[0], Mb[0]) and _bits(Ma[1], Mb[1])
    for k in GEOMETRY + ("shs",) + CAMERA:
        assert not torch.isnan(a[k]).any() and _bits(a[k], b[k]), k
    # a contribution walk between the forward and the backward changes nothing
    rs, res = _forward(inp, gpu_device)
    contributions_raw(res[-1], rs)
    c = backward_raw(res[-1], rs, _t(dc, gpu_device), _t(di, gpu_device), grad_out_median_depth=_t(gM, gpu_device),
                     camera_grads=True)
    torch.cuda.synchronize()
    for k in GEOMETRY + ("shs",) + CAMERA:
        assert _bits(c[k], a[k]), k


# ------------------------------------------------------------------------------------------------ 6. autograd
def test_autograd_surface(gpu_device):
    from gaussian_splatting_lightning_amd import GaussianRasterizer
    from gaussian_splatting_lightning_amd.rasterizer import backward_chunked, backward_raw
    name = "A"
    inp, dc, di = F.scene(name)
    dev = gpu_device
    t = _truth(name)
    n, W, H = AC.SCENES[name][:3]

    def leaves():
        lv = {k: _t(inp[k], dev).requires_grad_(True) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
        lv["means2D"] = torch.zeros(n, 3, device=dev, requires_grad=True)
        return lv

    def call(rast, lv, **kw):
        return rast(means3D=lv["means3D"], means2D=lv["means2D"], opacities=lv["opacities"], shs=lv["shs"],
                    scales=lv["scales"], rotations=lv["rotations"], **kw)

    # the two maps are the last outputs, after alpha, the feature image and the distortion map
    lv = leaves()
    out = call(GaussianRasterizer(settings_for(inp, dev), return_alpha=True, distortion="z", median_depth=True), lv,
               features=_t(F.inputs(name, C_FEAT)[0], dev))
    assert len(out) == 8 and out[5].shape == (1, H, W) and out[6].shape == (1, H, W) and out[7].shape == (1, H, W)
    assert out[6].requires_grad and out[6].dtype == torch.float32
    assert not out[7].requires_grad and out[7].dtype == torch.int32
    assert len(call(GaussianRasterizer(settings_for(inp, dev), return_alpha=True), leaves())) == 4
    # median_depth.sum().backward(): every non-candidate pixel hands 1 to its Gaussian's depth (scene A has no candidate)
    assert not t["candidate"].any()
    lv = leaves()
    color, radii, invd, md, mi = call(GaussianRasterizer(settings_for(inp, dev), median_depth=True), lv)
    md.sum().backward()
    dz, want = MC.gradient(name, t["index"], np.ones((1, H, W), f32), f64)
    rec = dict(means3D=rel_l2(lv["means3D"].grad.cpu().numpy(), want), bar=GRAD_CLEAN_TOL)
    for k in ("opacities", "scales", "rotations", "means2D", "shs"):
        assert lv[k].grad is None or float(lv[k].grad.abs().max()) == 0.0, k
    # the joint loss against backward_raw
    lv = leaves()
    color, radii, invd, md, mi = call(GaussianRasterizer(settings_for(inp, dev), median_depth=True), lv)
    gM = MC.upstream(name)
    ((color * _t(dc, dev)).sum() + (invd * _t(di, dev)).sum() + (md * _t(gM, dev)).sum()).backward()
    raw, _ = _run(inp, dev, dc=dc, di=di, gM=gM)
    for k in ("means3D", "shs", "opacities", "scales"):
        rec["joint_" + k] = rel_l2(lv[k].grad.cpu().numpy(), raw[k].cpu().numpy().reshape(lv[k].grad.shape))
    parity.record("median_autograd_A", "autograd", rec)
    print(rec)
    assert rec["means3D"] <= GRAD_CLEAN_TOL, rec
    for k in ("means3D", "shs", "opacities", "scales"):
        assert rec["joint_" + k] <= GRAD_TOL_ADHOC, (k, rec)
    # refusals
    rs, res = _forward(inp, dev)
    st = res[-1]
    with pytest.raises(NotImplementedError):
        backward_raw(st, rs, _t(dc, dev), _t(di, dev), grad_out_median_depth=_t(gM, dev), absgrad=True)
    with pytest.raises(NotImplementedError):
        backward_chunked(st, rs, _t(dc, dev), _t(di, dev), [(0, n, {})])
    with pytest.raises(NotImplementedError):
        call(GaussianRasterizer(rs, absgrad=True, median_depth=True), leaves())
    with pytest.raises(RuntimeError, match="needs a state"):
        backward_raw(_forward(inp, dev, median=False)[1][-1], rs, _t(dc, dev), grad_out_median_depth=_t(gM, dev))
    g = backward_raw(st, rs, _t(dc, dev), _t(di, dev), grad_out_median_depth=_t(gM, dev))  # the state still serves
    torch.cuda.synchronize()
    assert float(g["means3D"].abs().max()) > 0


def test_empty_scenes(gpu_device):
    from gaussian_splatting_lightning_amd.rasterizer import backward_raw, forward_raw
    inp, dc, di = F.scene("A")
    dev = gpu_device
    n, W, H = AC.SCENES["A"][:3]
    gM = MC.upstream("A")
    rs = settings_for(inp, dev)
    e = lambda *s: torch.zeros(0, *s, device=dev)  # noqa: E731
    color, radii, invd, md, mi, st = forward_raw(e(3), e(16, 3), None, e(1), e(3), e(4), None, rs, median_depth=True)
    g = backward_raw(st, rs, _t(dc, dev), _t(di, dev), grad_out_median_depth=_t(gM, dev))
    torch.cuda.synchronize()
    assert torch.all(md == 0) and torch.all(mi == -1) and torch.all(st.median.pos == -1)
    assert g["means3D"].shape == (0, 3)
    # every Gaussian behind the camera: nothing rendered, the same planes and zero gradients
    ph = np.asarray([0.0, 0.0, -1.0, 1.0]) @ np.linalg.inv(inp["viewmatrix"].astype(np.float64))
    behind = dict(inp, means3D=(inp["means3D"] * f32(0.01) + (ph[:3] / ph[3]).astype(f32)).astype(f32))
    g, (md, mi) = _run(behind, dev, dc=dc, di=di, gM=gM, camera_grads=True)
    assert torch.all(md == 0) and torch.all(mi == -1)
    assert torch.all(g["means3D"] == 0) and torch.all(g["viewmatrix"] == 0)


# ------------------------------------------------------------------------------------------------ 7. surface normals
def _hip_surface(inputs, rs, ratio, dev):
    from gaussian_splatting_lightning_amd import normal_consistency
    D, A, N, M, dE = (t.to(dev) for t in inputs)
    D, A, N, M = (t.detach().clone().requires_grad_(True) for t in (D, A, N, M))
    E = normal_consistency(D, A, N, rs, median_depth=M, depth_ratio=ratio)
    E.backward(dE)
    torch.cuda.synchronize()
    return E.detach(), D.grad, M.grad, A.grad, N.grad


def _compare_surface(case, inputs, rs, ratio, dev, tanfovx, tanfovy):
    got = _hip_surface(inputs, rs, ratio, dev)
    ref, bars = MC.surface_bars(inputs, ratio, tanfovx, tanfovy)
    errs = [NC.rel_l2(a, r) for a, r in zip(got, ref)]
    rec = {k: dict(rel_l2=e, bar=b) for k, e, b in zip(MC.SURFACE_QUANTITIES, errs, bars)}
    parity.record(case, f"surface_ratio_{ratio}", rec)
    print(case, ratio, rec)
    assert all(bool(torch.isfinite(t).all()) for t in got)
    for k, e, b in zip(MC.SURFACE_QUANTITIES, errs, bars):
        assert e <= b, f"{case} r={ratio} {k}: rel L2 {e:.3e} above the bar {b:.3e}"
    return got


def _normals_settings(H, W, tanfovx, tanfovy, dev):
    from gaussian_splatting_lightning_amd import GaussianRasterizationSettings
    return GaussianRasterizationSettings(H, W, tanfovx, tanfovy, torch.zeros(3, device=dev), 1.0,
                                         torch.eye(4, device=dev), torch.eye(4, device=dev), 0,
                                         torch.zeros(3, device=dev), False, False, False)


@pytest.mark.parametrize("ratio", [0.5, 1.0])
@pytest.mark.parametrize("case", MC.SURFACE_CASES, ids=lambda c: c.name)
def test_surface_normals_small_images(gpu_device, case, ratio):
    """One backward tile, and a partial tile whose halo crosses the image edge both ways."""
    rs = _normals_settings(case.H, case.W, case.tanfovx, case.tanfovy, gpu_device)
    got = _compare_surface(f"median_surface_{case.name}", MC.make_surface(case), rs, ratio, gpu_device,
                           case.tanfovx, case.tanfovy)
    assert bool(got[2].any()) and (ratio != 1.0 or (not got[1].any() and not got[3].any()))  # r = 1: all to the median


@pytest.mark.parametrize("ratio", [0.5, 1.0])
def test_surface_normals_on_rendered_maps(gpu_device, ratio):
    """Scene B rendered with the geometry features, alpha and the median depth: the loss map and the gradients to
    depth, median, alpha and normals against the float64 restatement on those maps; depth_ratio = 0 and
    median_depth=None are bitwise the call without a median."""
    from gaussian_splatting_lightning_amd import (GaussianRasterizer, depth_to_normal, geometry_features,
                                                  normal_consistency)
    dev = gpu_device
    inp = MC.scene("B")
    n, W, H = AC.SCENES["B"][:3]
    rs = settings_for(inp, dev)
    feats = geometry_features(_t(inp["means3D"], dev), _t(inp["scales"], dev), _t(inp["rotations"], dev), rs)
    with torch.no_grad():
        out = GaussianRasterizer(rs, return_alpha=True, median_depth=True)(
            means3D=_t(inp["means3D"], dev), means2D=None, opacities=_t(inp["opacities"], dev),
            shs=_t(inp["shs"], dev), scales=_t(inp["scales"], dev), rotations=_t(inp["rotations"], dev),
            features=feats)
    alpha, image, md = out[3], out[4], out[5]
    dE = torch.randn(1, H, W, generator=torch.Generator().manual_seed(17))
    inputs = tuple(t.cpu().contiguous() for t in (image[3:4], alpha, image[0:3], md)) + (dE,)
    got = _compare_surface("median_surface_B", inputs, rs, ratio, dev, inp["tanfovx"], inp["tanfovy"])
    assert bool(got[2].any())
    # the blend's normals are the forward's, and depth_ratio = 0 / no median are today's bits
    D, A, N, M = (t.to(dev) for t in inputs[:4])
    base = normal_consistency(D, A, N, rs)
    assert torch.equal(normal_consistency(D, A, N, rs, median_depth=M, depth_ratio=0.0), base)
    assert torch.equal(normal_consistency(D, A, N, rs, median_depth=None), base)
    assert torch.equal(depth_to_normal(D, A, rs, median_depth=M, depth_ratio=0.0), depth_to_normal(D, A, rs))
    assert not torch.equal(normal_consistency(D, A, N, rs, median_depth=M, depth_ratio=ratio), base)
    n_d = depth_to_normal(D, A, rs, median_depth=M, depth_ratio=ratio)
    flat = (n_d == 0).all(0, keepdim=True)
    want = torch.where(flat, torch.ones_like(A), 1 - A * (N * n_d).sum(0, keepdim=True))
    assert float((got[0] - want).abs().max()) <= 1e-6


def test_render_normal_consistency_with_depth_ratio(gpu_device):
    """render_normal_consistency(depth_ratio=1) through autograd: the loss reaches means3D through the median depth too,
    the same bits on a second run; without a ratio the call returns what it returned."""
    from gaussian_splatting_lightning_amd import GaussianRasterizer, render_normal_consistency
    dev = gpu_device
    inp = MC.scene("B")
    rs = settings_for(inp, dev)

    def run(ratio, **kw):
        lv = {k: _t(inp[k], dev).requires_grad_(True) for k in ("means3D", "opacities", "scales", "rotations")}
        out = render_normal_consistency(GaussianRasterizer(rs, return_alpha=True, **kw), lv["means3D"], None,
                                        lv["opacities"], shs=_t(inp["shs"], dev), scales=lv["scales"],
                                        rotations=lv["rotations"], **({} if ratio is None else dict(depth_ratio=ratio)))
        out[4].mean().backward()
        torch.cuda.synchronize()
        return out, {k: v.grad for k, v in lv.items()}

    (a, ga), (b, gb) = run(1.0, median_depth=True), run(1.0, median_depth=True)
    assert len(a) == 7 and a[6].shape == a[4].shape
    for k in ga:
        assert bool(torch.isfinite(ga[k]).all()) and bool(ga[k].any()) and torch.equal(ga[k], gb[k]), k
    (c, gc), (d, gd) = run(None), run(0.0)
    assert len(c) == 6 and len(d) == 6 and torch.equal(c[4], d[4]) and not torch.equal(c[4], a[4])
    for k in gc:
        assert torch.equal(gc[k], gd[k]), k
    with pytest.raises(ValueError, match="median_depth=True"):
        run(0.5)
