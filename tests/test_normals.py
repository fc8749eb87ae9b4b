"""Normal consistency on the GPU (csrc/gsr_normals.hip through normals.py) against the float64 restatement of
tests/normal_cases.py.

Image cases (H x W) and what each reaches:
  3x3          one interior pixel
  2x7, 5x1     no interior: E == 1 everywhere, every gradient exactly zero
  5x7          a few interior pixels, one workgroup
  37x53        odd sizes, a partial tile in both directions (the backward's tile is 64x16, the forward's block 64x4)
  17x130       rows that straddle tile and wave boundaries
  70x200       several tiles both ways, so every halo seam is interior somewhere
  37x53-hole   a rectangle of alpha == 0: E == 1 and exactly zero gradients inside it away from its rim
  37x53-plane  the depth image of a plane: n_d is the plane's normal and E = 1 - A^2, independent of the restatement

Bars.  Per case and quantity (E, dD, dA, dN; g, dmeans3D, drotations) the bar is 4 x the relative L2 error the float32
torch restatement makes on the CPU against float64 on the same input, with a floor of 4 * 2^-23 (C.bars,
C.geometry_bars); nothing is fitted to HIP output, and by the input conditions C.make() asserts no element is excluded.
Achieved errors and bars are recorded through tests.parity.
"""
import functools

import pytest
import torch

from tests import normal_cases as C
from tests import parity

pytestmark = pytest.mark.gpu


def _settings(case, dev, viewmatrix=None):
    from gaussian_splatting_lightning_amd import GaussianRasterizationSettings
    vm = torch.eye(4, device=dev) if viewmatrix is None else viewmatrix
    return GaussianRasterizationSettings(case.H, case.W, case.tanfovx, case.tanfovy, torch.zeros(3, device=dev), 1.0,
                                         vm, torch.eye(4, device=dev), 0, torch.zeros(3, device=dev), False, False,
                                         False)


def _hip(case, dev):
    """(E, dD, dA, dN) of normal_consistency under the case's upstream gradient."""
    from gaussian_splatting_lightning_amd import normal_consistency
    D, A, N, dE = (t.to(dev) for t in C.make(case))
    D, A, N = (t.requires_grad_(True) for t in (D, A, N))
    E = normal_consistency(D, A, N, _settings(case, dev))
    E.backward(dE)
    torch.cuda.synchronize()
    return E.detach(), D.grad, A.grad, N.grad


@functools.lru_cache(maxsize=None)
def _hip_cached(case, dev):
    return _hip(case, dev)


def _compare(case, got, ref, bars, names, kind):
    errs = [C.rel_l2(a, r) for a, r in zip(got, ref)]
    record = {k: {"rel_l2": e, "bar": b} for k, e, b in zip(names, errs, bars)}
    print(case.name, record)
    parity.record(f"normals-{case.name}", kind, record)
    for name, e, b in zip(names, errs, bars):
        assert e <= b, f"{case.name} {name}: rel L2 {e:.3e} above the bar {b:.3e}"


IMAGE_CASES = [c for c in C.CASES if c.plane is None]


@pytest.mark.parametrize("case", IMAGE_CASES, ids=lambda c: c.name)
def test_consistency_forward_backward_parity(gpu_device, case):
    got = _hip_cached(case, gpu_device)
    assert all(bool(torch.isfinite(t).all()) for t in got)
    assert got[0].shape == (1, case.H, case.W) and got[3].shape == (3, case.H, case.W)
    if case.H < 3 or case.W < 3:  # no interior
        assert bool((got[0] == 1).all())
        assert not got[1].any() and not got[2].any() and not got[3].any()
        return
    E = got[0][0]
    border = torch.ones_like(E, dtype=torch.bool)
    border[1:-1, 1:-1] = False
    assert bool((E[border] == 1).all()) and not got[3][:, border].any()
    if case.hole is not None:
        y0, y1, x0, x1 = case.hole
        inner = (slice(None), slice(y0 + 1, y1 - 1), slice(x0 + 1, x1 - 1))
        assert bool((got[0][inner] == 1).all()), "E == 1 exactly inside the hole"
        for t in got[1:]:
            assert not t[inner].any(), "exactly zero gradients inside the hole"
        hole = (slice(None), slice(y0, y1), slice(x0, x1))
        assert not got[1][hole].any() and not got[2][hole].any()  # alpha == 0 takes no gradient through d
    _compare(case, got, C.reference(case), C.bars(case), C.QUANTITIES, "consistency")


def test_analytic_plane(gpu_device):
    """n_d within 1e-5 of the plane's normal at every interior pixel, E within the case's bar of 1 - A^2."""
    from gaussian_splatting_lightning_amd import depth_to_normal
    case = C.BY_NAME["37x53-plane"]
    D, A, _, _ = (t.to(gpu_device) for t in C.make(case))
    n_d = depth_to_normal(D, A, _settings(case, gpu_device)).cpu().double()
    n = torch.tensor(case.plane[:3], dtype=torch.float64).view(3, 1, 1)
    err = float((n_d[:, 1:-1, 1:-1] - n).abs().max())
    want = (1 - A.cpu().double() ** 2)[:, 1:-1, 1:-1]
    e = C.rel_l2(_hip_cached(case, gpu_device)[0][:, 1:-1, 1:-1], want)
    record = {"n_d_max_abs": err, "n_d_bar": 1e-5, "E_rel_l2": e, "E_bar": C.bars(case)[0]}
    print(case.name, record)
    parity.record(f"normals-{case.name}", "plane", record)
    assert err <= 1e-5, record
    assert e <= C.bars(case)[0], record
    assert not n_d[:, 0].any() and not n_d[:, -1].any() and not n_d[:, :, 0].any() and not n_d[:, :, -1].any()


@pytest.mark.parametrize("name", ["3x3", "2x7", "37x53-hole", "70x200"])
def test_depth_to_normal_is_the_forwards_output(gpu_device, name):
    """depth_to_normal equals the forward's optional n_d bit for bit, and E is what n_d gives."""
    from gaussian_splatting_lightning_amd import _native, depth_to_normal
    from gaussian_splatting_lightning_amd.rasterizer import _stream_handle
    case = C.BY_NAME[name]
    D, A, N, _ = (t.to(gpu_device) for t in C.make(case))
    n_d, E = torch.full((3, case.H, case.W), 7.0, device=gpu_device), torch.full_like(D, 7.0)
    lib = _native.load()
    _native.check(lib.gsr_normal_consistency_forward(case.H, case.W, case.tanfovx, case.tanfovy, D.data_ptr(),
                                                     A.data_ptr(), N.data_ptr(), E.data_ptr(), n_d.data_ptr(),
                                                     _stream_handle(gpu_device)), "gsr_normal_consistency_forward")
    assert torch.equal(depth_to_normal(D, A, _settings(case, gpu_device)), n_d)
    assert torch.equal(E, _hip_cached(case, gpu_device)[0])
    ref = C.depth_normals(*(t.double() for t in C.make(case)[:2]), case.tanfovx, case.tanfovy)
    assert bool(((n_d.cpu() == 0).all(0) == (ref == 0).all(0)).all())  # zero exactly where the definition's is
    if case.H >= 3 and case.W >= 3:  # the bar as everywhere: the float32 restatement's own error, times BAR_FACTOR
        bar = C.bar_of(C.depth_normals(*C.make(case)[:2], case.tanfovx, case.tanfovy), ref)
        err = C.rel_l2(n_d, ref)
        parity.record(f"normals-{case.name}", "n_d", {"rel_l2": err, "bar": bar})
        assert err <= bar, (err, bar)


def _hip_geometry(case, dev):
    from gaussian_splatting_lightning_amd import geometry_features
    means, scales, rots, vm, dg = (t.to(dev) for t in C.make_geometry(case))
    means, scales, rots = (t.requires_grad_(True) for t in (means, scales, rots))
    g = geometry_features(means, scales, rots, vm)
    g.backward(dg)
    torch.cuda.synchronize()
    return g.detach(), means.grad, rots.grad, scales.grad


@functools.lru_cache(maxsize=None)
def _hip_geometry_cached(case, dev):
    return _hip_geometry(case, dev)


@pytest.mark.parametrize("case", C.GEOMETRY_CASES, ids=lambda c: c.name)
def test_geometry_features_parity(gpu_device, case):
    g, dmeans, drots, dscales = _hip_geometry_cached(case, gpu_device)
    assert g.shape == (case.P, 4)
    assert dscales is None or not dscales.any(), "scales take no gradient"
    _compare(case, (g, dmeans, drots), C.geometry_reference(case), C.geometry_bars(case), C.GEOMETRY_QUANTITIES,
             "geometry")
    # the flip is the definition's on every row
    assert bool(((g[:, :3].cpu().double() * C.geometry_reference(case)[0][:, :3]).sum(1) > 0.99).all())


def test_geometry_rows_are_independent(gpu_device):
    """Permuting the Gaussians permutes the output and the gradients bit for bit; a settings object is the viewmatrix."""
    from gaussian_splatting_lightning_amd import geometry_features
    case = C.GEOMETRY_CASES[-1]
    perm = torch.randperm(case.P, generator=torch.Generator().manual_seed(3)).to(gpu_device)
    means, scales, rots, vm, dg = (t.to(gpu_device) for t in C.make_geometry(case))
    pm, ps, pr = (t[perm].contiguous().requires_grad_(True) for t in (means, scales, rots))
    rs = _settings(C.CASES[0], gpu_device, viewmatrix=vm)
    g = geometry_features(pm, ps, pr, rs)
    g.backward(dg[perm].contiguous())
    base = _hip_geometry_cached(case, gpu_device)
    assert torch.equal(g.detach(), base[0][perm])
    assert torch.equal(pm.grad, base[1][perm]) and torch.equal(pr.grad, base[2][perm])
    assert ps.grad is None or not ps.grad.any()


def test_backwards_are_deterministic(gpu_device):
    for case in (C.BY_NAME["70x200"], C.BY_NAME["37x53-hole"]):
        for x, y in zip(_hip_cached(case, gpu_device), _hip(case, gpu_device)):
            assert torch.equal(x, y)
    case = C.GEOMETRY_CASES[-1]
    for x, y in zip(_hip_geometry_cached(case, gpu_device)[:3], _hip_geometry(case, gpu_device)[:3]):
        assert torch.equal(x, y)


def _end_to_end(dev):
    from gaussian_splatting_lightning_amd import (GaussianRasterizationSettings, GaussianRasterizer,
                                                  render_normal_consistency)
    from gaussian_splatting_lightning_amd.synthetic import make_camera, make_scene
    W, H = 96, 64
    cam, scene = make_camera(W, H).to(dev), make_scene(300, sh_degree=1, seed=4)
    rs = GaussianRasterizationSettings(H, W, cam.tanfovx, cam.tanfovy, torch.zeros(3, device=dev), 1.0,
                                       cam.viewmatrix, cam.projmatrix, 1, cam.campos, False, False, False)
    leaves = dict(means3D=scene.means3D * 1.5, opacities=scene.opacities, scales=scene.scales * 2.0,
                  rotations=scene.rotations)
    leaves = {k: v.to(dev).contiguous().requires_grad_(True) for k, v in leaves.items()}
    shs = scene.shs.to(dev)
    color, radii, invdepth, alpha, E, normals = render_normal_consistency(
        GaussianRasterizer(rs, return_alpha=True), leaves["means3D"], None, leaves["opacities"], shs=shs,
        scales=leaves["scales"], rotations=leaves["rotations"])
    E.mean().backward()
    torch.cuda.synchronize()
    plain = GaussianRasterizer(rs)(means3D=leaves["means3D"].detach(), means2D=None,
                                   opacities=leaves["opacities"].detach(), shs=shs, scales=leaves["scales"].detach(),
                                   rotations=leaves["rotations"].detach())[0]
    return dict(color=color.detach(), radii=radii, alpha=alpha.detach(), E=E.detach(), normals=normals.detach(),
                plain=plain, grads={k: v.grad for k, v in leaves.items()}, shape=(H, W))


def test_end_to_end_render(gpu_device):
    """A few hundred Gaussians through render_normal_consistency and E.mean().backward(): finite gradients, non-zero
    somewhere on each parameter, exactly zero for the Gaussians the view culls, the same bits on a second run, and the
    colour of a plain render of the same scene."""
    a, b = _end_to_end(gpu_device), _end_to_end(gpu_device)
    H, W = a["shape"]
    assert a["E"].shape == (1, H, W) and a["normals"].shape == (3, H, W) and a["alpha"].shape == (1, H, W)
    assert bool(torch.isfinite(a["E"]).all()) and bool((a["E"] != 1).any())
    culled = a["radii"] == 0
    assert bool(culled.any()) and bool((~culled).any())
    for k, g in a["grads"].items():
        assert g is not None and bool(torch.isfinite(g).all()), k
        assert bool(g.any()), f"{k}: the loss reaches it"
        assert not g[culled].any(), f"{k}: a culled Gaussian takes no gradient"
        assert torch.equal(g, b["grads"][k]), f"{k}: the same bits on a second run"
    assert torch.equal(a["E"], b["E"])
    assert torch.equal(a["color"], a["plain"]), "the feature changes no existing result"
