"""Mip-Splatting's 3D smoothing filter on the GPU (csrc/gsr_mipfilter.hip through mipfilter.py, gaussian_model.py and
ply.py) against the float64 restatement of tests/mipfilter_cases.py.

Bars.
* seen is exact: the scene generators keep every (Gaussian, camera) pair 1e-4 relative or more from the thresholds.
* rate and zmin: the derived per-Gaussian bound of mipfilter_cases.rate_bars (the fp32 rounding of z, plus 2 ulp for fx
  and the division); the fp32 CPU restatement's error is recorded beside it.  filter_3D: the same bound carried through
  sqrt(variance) / rate (or zmin / max fx), plus 2 ulp for those two operations.
* activations and their gradients: the error against the float64 restatement on the fp32 inputs; the bar is twice the
  error the fp32 CPU restatement of the ratio form makes on the same inputs (computed every run), at least 4 fp32 ulp
  (mcmc_cases.bar).  Forward: largest relative error; gradients: relative L2 over the tensor.
Achieved errors and bars are recorded through tests.parity (profiles/parity_mipfilter.json is one run).
"""
import numpy as np
import pytest
import torch

from tests import mipfilter_cases as C
from tests import parity

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -23


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---------------------------------------------------------------------------------------- sampling rate

def check_rates(name, means, cams, got, near=C.NEAR, margin=C.MARGIN):
    rate, zmin, seen = (t.cpu() for t in got)
    r64, z64, s64 = C.sampling_rate(means, cams, near, margin)
    r32, z32, _ = C.sampling_rate(means, cams, near, margin, dtype=torch.float32)
    rb, zb = C.rate_bars(means, cams, near, margin)
    vis = s64 > 0
    assert seen.dtype == torch.int32 and torch.equal(seen, s64), name
    assert bool((rate[~vis] == 0).all()) and bool(torch.isinf(zmin[~vis]).all()) and bool((zmin[~vis] > 0).all()), name
    worst = lambda err, b: float((err[vis] / b[vis]).max()) if bool(vis.any()) else 0.0  # noqa: E731
    res = dict(P=int(means.shape[0]), V=int(cams["viewmatrix"].shape[0]), seen_mismatches=0,
               seen_none=int((~vis).sum()), seen_all=int((s64 == cams["viewmatrix"].shape[0]).sum()),
               rate_error_over_bar=worst((rate.double() - r64).abs(), rb),
               zmin_error_over_bar=worst((zmin.double() - z64).abs(), zb),
               rate_max_rel=C.max_rel(rate[vis], r64[vis]) if bool(vis.any()) else 0.0,
               rate_bar_max_rel=float((rb[vis] / r64[vis]).max()) if bool(vis.any()) else 0.0,
               fp32_cpu_rate_error_over_bar=worst((r32.double() - r64).abs(), rb),
               fp32_cpu_zmin_error_over_bar=worst((z32.double() - z64).abs(), zb))
    print(name, res)
    parity.record(f"mipfilter_rate_{name}", "rate", res)
    assert res["rate_error_over_bar"] <= 1.0 and res["zmin_error_over_bar"] <= 1.0, (name, res)


@pytest.mark.parametrize("name", C.SCENES)
def test_sampling_rate(gpu_device, name):
    """P = 1000, V = 5 (a partial last block, every visibility category); P = 257, V = 1; P = 1, V = 1; P = 513,
    V = 300 with three focals and image sizes.  Both forms of `cameras` give the same bits, and two calls do."""
    from gaussian_splatting_lightning_amd.mipfilter import sampling_rate
    means, cams = C.scene(name)
    dmeans = means.to(gpu_device)
    got = sampling_rate(dmeans, C.cameras_to(cams, gpu_device))
    check_rates(name, means, cams, got)
    again = sampling_rate(dmeans, cams if name == "ring300" else C.as_settings(cams))  # host tensors / settings
    for a, b in zip(got, again):
        assert same_bits(a, b), name


def test_sampling_rate_empty_and_other_planes(gpu_device):
    from gaussian_splatting_lightning_amd.mipfilter import compute_3d_filter, sampling_rate
    means, cams = C.scene("ring5")
    rate, zmin, seen = sampling_rate(torch.zeros(0, 3, device=gpu_device), cams)
    assert rate.shape == zmin.shape == seen.shape == (0,) and seen.dtype == torch.int32 and rate.is_cuda
    assert compute_3d_filter(torch.zeros(0, 3, device=gpu_device), cams).shape == (0, 1)
    # another near plane and no margin: the arguments reach the kernel (the clearance is asserted for them too)
    near, margin = 2.0, 0.0
    assert float(C.thresholds(means, cams, near, margin)[2].min()) > C.CLEARANCE
    got = sampling_rate(means.to(gpu_device), cams, near=near, margin=margin)
    check_rates("ring5_near2_margin0", means, cams, got, near, margin)
    assert not torch.equal(got[2].cpu(), C.sampling_rate(means, cams)[2])


def test_boundary_points(gpu_device):
    """One point on each side of each threshold, 1e-3 relative away: z = near (1 +- 1e-3), |x| = limx z (1 +- 1e-3) for
    both signs, the same for y.  The decisions are exact."""
    from gaussian_splatting_lightning_amd.mipfilter import sampling_rate
    means, cams, seen = C.boundary_points()
    got = sampling_rate(means.to(gpu_device), cams)
    assert got[2].cpu().tolist() == seen.tolist()
    check_rates("boundary", means, cams, got)


@pytest.mark.parametrize("mode", ["per_camera", "shared_focal"])
def test_compute_3d_filter(gpu_device, mode):
    from gaussian_splatting_lightning_amd.mipfilter import compute_3d_filter
    res = {}
    for name in ("ring5", "ring300"):
        means, cams = C.scene(name)
        f = compute_3d_filter(means.to(gpu_device), C.cameras_to(cams, gpu_device), mode=mode)
        assert f.shape == (means.shape[0], 1) and f.dtype == torch.float32 and f.is_contiguous()
        want = C.filter_3d(means, cams, mode=mode)
        rate, zmin, seen = C.sampling_rate(means, cams)
        rb, zb = C.rate_bars(means, cams)
        vis = seen > 0
        # the relative error of rate (or zmin) carries over, plus an ulp each for the scale and the division
        rel_bar = (rb[vis] / rate[vis] if mode == "per_camera" else zb[vis] / zmin[vis]) + 2 * ULP
        err = ((f.cpu().double() - want)[vis, 0].abs() / want[vis, 0])
        res[name] = dict(error_over_bar=float((err / rel_bar).max()), max_rel=float(err.max()))
        assert res[name]["error_over_bar"] <= 1.0, (name, mode, res[name])
        # the unseen rows take the largest value among the seen ones, bit for bit
        assert int((~vis).sum()) > 0 and bool((f.cpu()[~vis, 0] == f.cpu()[vis, 0].max()).all()), name
    print(mode, res)
    parity.record(f"mipfilter_filter_{mode}", "filter_3D", res)
    means, cams = C.scene("unseen")  # a scene no camera sees: the identity
    f = compute_3d_filter(means.to(gpu_device), cams, mode=mode)
    assert f.shape == (65, 1) and bool((f == 0).all())


def test_filter_modes_agree_for_equal_focals(gpu_device):
    from gaussian_splatting_lightning_amd.mipfilter import compute_3d_filter
    means, cams = C.scene("ring5")
    a = compute_3d_filter(means.to(gpu_device), cams, mode="per_camera")
    b = compute_3d_filter(means.to(gpu_device), cams, mode="shared_focal")
    assert C.max_rel(a, b) <= 4 * ULP  # fx / z inverted against z / fx: two roundings each
    v = compute_3d_filter(means.to(gpu_device), cams, variance=0.8)
    assert C.max_rel(v, 2 * a) <= 2 * ULP


# ---------------------------------------------------------------------------------------- filtered activations

def run_activations(case, N, dev):
    from gaussian_splatting_lightning_amd.mipfilter import FilteredGaussianActivations
    ref = C.activation_reference(case, N)
    leaves = [t.to(dev).requires_grad_(True) for t in ref["inputs"][:3]]
    out = FilteredGaussianActivations.apply(*leaves, ref["inputs"][3].to(dev))
    torch.autograd.backward(out, [u.to(dev) for u in ref["ups"]])
    return ref, leaves, out


@pytest.mark.parametrize("N", C.SIZES)
@pytest.mark.parametrize("case", C.RANGES)
def test_filtered_activations(gpu_device, case, N):
    """Forward and backward at N = 1000 and N = 1 over the five ranges (mipfilter_cases.activation_inputs).  Everywhere
    the rotation outputs are activate()'s bit for bit; with f = 0 all three are."""
    from gaussian_splatting_lightning_amd.activations import activate
    ref, leaves, out = run_activations(case, N, gpu_device)
    s, o, q, f = (t.to(gpu_device) for t in ref["inputs"])
    plain = activate(s, o, q)
    assert out[0].shape == (N, 3) and out[1].shape == (N, 1) and out[2].shape == (N, 4)
    assert same_bits(out[2], plain[2])
    if case == "zero":
        assert same_bits(out[0], plain[0]) and same_bits(out[1], plain[1])
    if case == "needle":
        assert bool((out[1] > 0).all()) and float(out[1].detach().max()) < 1e-12
    got = dict(scales=C.max_rel(out[0].detach().cpu(), ref["out64"][0]),
               opacities=C.max_rel(out[1].detach().cpu(), ref["out64"][1]),
               d_scaling=C.rel_l2(leaves[0].grad.cpu(), ref["g64"][0]),
               d_opacity=C.rel_l2(leaves[1].grad.cpu(), ref["g64"][1]),
               d_rotation=C.rel_l2(leaves[2].grad.cpu(), ref["g64"][2]))
    res = {k: dict(error=got[k], fp32_cpu_error=ref["fp32_error"][k], bar=C.bar(ref["fp32_error"][k])) for k in got}
    print(case, N, res)
    parity.record(f"mipfilter_activations_{case}_N{N}", "activations", res)
    for k, v in res.items():
        assert np.isfinite(v["error"]) and v["error"] <= v["bar"], (case, N, k, v)
    # the compensation keeps the Gaussian's integral, on the GPU's own outputs: o' prod s' = o prod s, to the roundings
    # of the seven operations between them (three ratios, their product, the products on either side)
    kept = C.max_rel(out[1].detach().double() * out[0].detach().double().prod(1, keepdim=True),
                     plain[1].double() * plain[0].double().prod(1, keepdim=True))
    parity.record(f"mipfilter_activations_{case}_N{N}", "integral", dict(error=kept, bar=12 * ULP))
    assert kept <= 12 * ULP, (case, N, kept)


def test_filtered_activations_autograd_and_determinism(gpu_device):
    """None incoming gradients are zeros, as in GaussianActivations; the filter takes no gradient; two calls give the
    same bits; the functional forms and `out=` give what the Function gives."""
    from gaussian_splatting_lightning_amd.mipfilter import (FilteredGaussianActivations, activate_filtered,
                                                            activate_filtered_backward)
    ref, leaves, out = run_activations("ordinary", 1000, gpu_device)
    _, leaves2, out2 = run_activations("ordinary", 1000, gpu_device)
    for a, b in zip(list(out) + [t.grad for t in leaves], list(out2) + [t.grad for t in leaves2]):
        assert same_bits(a.detach(), b.detach())
    s, o, q, f = (t.to(gpu_device) for t in ref["inputs"])
    ups = [u.to(gpu_device) for u in ref["ups"]]
    bufs = (torch.empty_like(s), torch.empty_like(o), torch.empty_like(q))
    assert activate_filtered(s, o, q, f.reshape(-1), out=bufs) is bufs  # filter_3D (N) as well as (N,1)
    for a, b in zip(bufs, out):
        assert same_bits(a, b.detach())
    for a, b in zip(activate_filtered_backward(s, o, q, f, *ups), leaves):
        assert same_bits(a, b.grad)
    # only the opacities are used: the other two incoming gradients are None
    fl = f.clone().requires_grad_(True)
    lv = [t.clone().requires_grad_(True) for t in (s, o, q)]
    FilteredGaussianActivations.apply(*lv, fl)[1].backward(ups[1])
    zero = torch.zeros_like
    want = activate_filtered_backward(s, o, q, f, zero(ups[0]), ups[1], zero(ups[2]))
    for a, b in zip(lv, want):
        assert same_bits(a.grad, b)
    assert fl.grad is None
    assert bool((lv[2].grad == 0).all()) and bool((lv[0].grad != 0).any())  # o' depends on the scaling
    with pytest.raises(RuntimeError):  # rotation storage 4 B past a 16-B boundary is refused, not misread
        buf = torch.empty(1000 * 4 + 1, device=gpu_device)
        qm = buf[1:].view(1000, 4)
        qm.copy_(q)
        activate_filtered(s, o, qm, f)


# ---------------------------------------------------------------------------------------- integration

def test_render_through_filtered_activations(gpu_device):
    """A 64 x 64 render of a synthetic scene of 500 Gaussians fed by FilteredGaussianActivations: backward() reaches
    _scaling and _opacity with finite values, and they match the same rasterizer fed by the torch formulas.  The bar is
    the activation gradients' (twice the fp32 CPU restatement's relative L2 error on these inputs and this upstream, at
    least 4 ulp) times the norm of the upstream gradient at the activated tensors: the two routes hand the rasterizer
    scales and opacities that differ in the last bits, and every entry of the activations' Jacobian is below one."""
    from gaussian_splatting_lightning_amd.mipfilter import FilteredGaussianActivations, compute_3d_filter
    from gaussian_splatting_lightning_amd.rasterizer import GaussianRasterizationSettings, rasterize_gaussians
    from gaussian_splatting_lightning_amd.synthetic import make_camera, make_scene, make_upstream
    dev = gpu_device
    W = H = 64
    cam = make_camera(W, H).to(dev)
    sc = make_scene(500, sh_degree=1, seed=5).to(dev)
    settings = GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=torch.zeros(3, device=dev),
        scale_modifier=1.0, viewmatrix=cam.viewmatrix, projmatrix=cam.projmatrix, sh_degree=1, campos=cam.campos,
        prefiltered=False, debug=False, antialiasing=True)
    f = compute_3d_filter(sc.means3D, [settings])
    assert float(f.min()) > 0
    raw = (torch.log(sc.scales), torch.log(sc.opacities / (1 - sc.opacities)), sc.rotations * 1.7)
    dcolor = make_upstream(W, H, seed=5)[0].to(dev)

    def render(activate):
        leaves = [t.clone().requires_grad_(True) for t in raw]
        act = activate(*leaves)
        for t in act:
            t.retain_grad()
        img = rasterize_gaussians(sc.means3D, torch.zeros_like(sc.means3D), sc.shs, None, act[1], act[0], act[2],
                                  None, settings)[0]
        (img * dcolor).sum().backward()
        return leaves, act, img

    def torch_formulas(a, b, q):
        s = torch.exp(a)
        sf = torch.sqrt(s * s + f * f)
        return sf, torch.sigmoid(b) * (s / sf).prod(1, keepdim=True), torch.nn.functional.normalize(q)

    ours, act, img = render(lambda a, b, q: FilteredGaussianActivations.apply(a, b, q, f))
    theirs, act_t, img_t = render(torch_formulas)
    assert float(img.detach().abs().max()) > 0.05  # something was rendered
    ups = [t.grad.cpu() for t in act]
    inp = [t.cpu() for t in raw] + [f.cpu()]
    g64 = C.activation_grads(*inp, ups)
    g32 = C.activation_grads(*inp, ups, dtype=torch.float32)
    res = {}
    for k, name in enumerate(("d_scaling", "d_opacity")):
        g, t = ours[k].grad, theirs[k].grad
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, name
        rel_bar = C.bar(C.rel_l2(g32[k], g64[k]))
        upstream_norm = float(torch.cat([ups[0].reshape(-1), ups[1].reshape(-1)]).double().norm())
        res[name] = dict(error=float((g - t).double().norm()), bar=rel_bar * upstream_norm, rel_bar=rel_bar,
                         upstream_norm=upstream_norm, gradient_norm=float(t.double().norm()),
                         against_float64_rel_l2=C.rel_l2(g.cpu(), g64[k]))
    print(res)
    parity.record("mipfilter_render_64x64", "gradients", res)
    for name, v in res.items():
        assert v["error"] <= v["bar"], (name, v)


# ---------------------------------------------------------------------------------------- model and PLY

def make_model(N, dev, seed=0):
    from gaussian_splatting_lightning_amd.gaussian_model import GaussianModel
    rng = np.random.default_rng(seed)
    g = GaussianModel(sh_degree=1, spatial_scale=1.0, device=dev)
    g.create_from_points(torch.tensor(1.5 * rng.normal(size=(N, 3)), dtype=torch.float32),
                         torch.tensor(rng.uniform(0, 1, (N, 3)), dtype=torch.float32))
    with torch.no_grad():
        g._rotation.copy_(torch.tensor(rng.normal(size=(N, 4)), dtype=torch.float32))
        g._opacity.copy_(torch.tensor(rng.normal(size=(N, 1)), dtype=torch.float32))
        g._features_rest.copy_(torch.tensor(rng.normal(size=(N, 3, 3)), dtype=torch.float32))
    return g


def test_model_buffer_getters_and_stale_filter(gpu_device):
    from gaussian_splatting_lightning_amd.activations import GaussianActivations
    from gaussian_splatting_lightning_amd.mipfilter import FilteredGaussianActivations, compute_3d_filter
    g = make_model(600, gpu_device)
    cams = C.ring_cameras(5)
    with pytest.raises(RuntimeError, match="compute_3d_filter"):
        g.get_scaling_with_3D_filter()
    f = g.compute_3d_filter(cams)
    assert f is g.filter_3D and f.shape == (600, 1) and "filter_3D" in dict(g.named_buffers())
    assert same_bits(f, compute_3d_filter(g._xyz.detach(), cams))
    assert not same_bits(f, g.compute_3d_filter(cams, mode="shared_focal", variance=0.3)) and g.filter_3D.shape == (600, 1)
    f = g.compute_3d_filter(cams)
    want = FilteredGaussianActivations.apply(g._scaling, g._opacity, g._rotation, f)
    got = g.get_activated(filter_3d=True)
    for a, b in zip(got, want):
        assert same_bits(a.detach(), b.detach())
    assert same_bits(g.get_scaling_with_3D_filter().detach(), want[0].detach())
    assert same_bits(g.get_opacity_with_3D_filter().detach(), want[1].detach())
    for a, b in zip(g.get_activated(), GaussianActivations.apply(g._scaling, g._opacity, g._rotation)):
        assert same_bits(a.detach(), b.detach())
    (got[0].sum() + got[1].sum()).backward()
    assert bool(torch.isfinite(g._scaling.grad).all()) and float(g._opacity.grad.abs().max()) > 0
    # the number of Gaussians changes: the old buffer is refused until the filter is recomputed
    g.xyz_grad_accum.fill_(1.0)
    g.xyz_grad_count.fill_(1.0)
    g.densify_and_prune(0.0002, 0.01, 0.005, 0.5)
    assert g._xyz.shape[0] != 600 and g.filter_3D.shape[0] == 600
    with pytest.raises(RuntimeError, match="filter_3D of 600 rows.*compute_3d_filter"):
        g.get_activated(filter_3d=True)
    N = g._xyz.shape[0]
    assert g.compute_3d_filter(cams).shape == (N, 1) and g.get_opacity_with_3D_filter().shape == (N, 1)
    assert g.add_new(N + 7, growth=1.05) == 7
    with pytest.raises(RuntimeError, match="compute_3d_filter"):
        g.get_scaling_with_3D_filter()
    with pytest.raises(RuntimeError, match="compute_3d_filter"):
        g.save_ply("unused.ply", with_filter=True)
    g.compute_3d_filter(cams)
    assert g.get_scaling_with_3D_filter().shape == (N + 7, 3)


def test_ply_round_trip_with_filter(gpu_device, tmp_path):
    from gaussian_splatting_lightning_amd import ply
    from gaussian_splatting_lightning_amd.gaussian_model import GaussianModel
    g = make_model(300, gpu_device, seed=1)
    g.compute_3d_filter(C.ring_cameras(5))
    plain, through, filtered = (str(tmp_path / n) for n in ("plain.ply", "through.ply", "filtered.ply"))
    # without the filter: the bytes of the unchanged path (the writer called as before this argument existed)
    assert g.save_ply(plain)
    assert ply.save_ply(through, g._xyz, g._features_dc, g._features_rest, g._opacity, g._scaling, g._rotation)
    a, b = open(plain, "rb").read(), open(through, "rb").read()
    assert a == b and b"filter_3D" not in a
    assert a.startswith(ply.header_bytes(300, ply.attribute_names(3, 9)))
    assert "filter_3D" not in ply.load_ply(plain, device=gpu_device)
    # with it: one more float property after rot_3, the other columns unchanged
    assert g.save_ply(filtered, with_filter=True)
    c = open(filtered, "rb").read()
    names = ply.attribute_names(3, 9) + ["filter_3D"]
    head = ply.header_bytes(300, names)
    assert c.startswith(head) and len(c) == len(head) + 300 * 4 * len(names)
    rec = np.frombuffer(c[len(head):], dtype="<f4").reshape(300, len(names))
    old = np.frombuffer(a[len(a) - 300 * 4 * (len(names) - 1):], dtype="<f4").reshape(300, len(names) - 1)
    assert np.array_equal(rec[:, :-1].view(np.int32), old.view(np.int32))
    assert np.array_equal(rec[:, -1], g.filter_3D.cpu().numpy()[:, 0])
    d = ply.load_ply(filtered, device=gpu_device)
    assert d["filter_3D"].shape == (300, 1) and same_bits(d["filter_3D"], g.filter_3D)
    h = GaussianModel(sh_degree=1, device=gpu_device)
    h.load_ply(filtered)
    assert same_bits(h.filter_3D, g.filter_3D) and same_bits(h._scaling.detach(), g._scaling.detach())
    for x, y in zip(h.get_activated(filter_3d=True), g.get_activated(filter_3d=True)):
        assert same_bits(x.detach(), y.detach())
    h.load_ply(plain)  # a plain checkpoint resets the buffer
    assert h.filter_3D is None


def test_save_fused_ply(gpu_device, tmp_path):
    """The fused checkpoint is a plain 3DGS file: loaded with compat="official" and activated plainly it gives s' and
    o'.  Bar: the activation bar of these inputs, plus what storing x = log(s') or logit(o') in fp32 costs: the
    logarithm is good to an ulp of x, which the exponential turns into |x| 2^-23 relative (the sigmoid into at most
    that), and an ulp each for the exponential and the quotient inside the logit."""
    from gaussian_splatting_lightning_amd import ply
    from gaussian_splatting_lightning_amd.gaussian_model import GaussianModel
    g = make_model(300, gpu_device, seed=2)
    g.compute_3d_filter(C.ring_cameras(5))
    path = str(tmp_path / "fused.ply")
    assert g.save_fused_ply(path)
    assert b"filter_3D" not in open(path, "rb").read()[:4096]
    h = GaussianModel(sh_degree=1, device=gpu_device)
    h.load_ply(path)
    assert h.filter_3D is None and same_bits(h._rotation.detach(), g._rotation.detach())
    inp = [t.detach().cpu() for t in (g._scaling, g._opacity, g._rotation, g.filter_3D)]
    s64, o64, _ = C.activations(*inp)
    s32, o32, _ = C.activations(*inp, dtype=torch.float32)
    got_s, got_o, _ = h.get_activated()
    res = {}
    for name, got, want, w32, raw in (("scales", got_s, s64, s32, torch.log(s64)),
                                      ("opacities", got_o, o64, o32, torch.log(o64 / (1 - o64)))):
        stored = float(raw.abs().max()) * ULP + 2 * ULP
        res[name] = dict(error=C.max_rel(got.detach().cpu(), want), bar=C.bar(C.max_rel(w32, want)) + stored)
    print(res)
    parity.record("mipfilter_fused_ply", "activated", res)
    for name, v in res.items():
        assert v["error"] <= v["bar"], (name, v)
