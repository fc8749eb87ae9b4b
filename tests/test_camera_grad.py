"""Camera gradients (dL/dviewmatrix, dL/dprojmatrix, dL/dcampos) of the HIP backward on the GPU: parity with the
reference's autograd gradients (tests/golden/camgrad.npz, tests/golden/make_golden_camera.py), the translation
identity, determinism, the chunked backward and the autograd route.

Bars.  Reference parity: 2e-5 relative L2 per tensor, the project's reference-gradient bar; the
reference's own float32 result is within 0.3e-6 .. 2.7e-6 of its float64 one on these cases.  Translation identity:
|residual| <= 1e-6 (sum_g |dL/dmeans3D_g| + |dL/dcampos|) per component -- the reference's float32 gradients leave
1e-8 of that scale, a dropped term leaves O(1); stated on Gaussians inside the EWA clamp (identity_scene)."""
import functools

import numpy as np
import pytest
import torch

from tests import parity
from tests.camera_cases import (BIG_CASE, BIG_GAUSSIAN_TILES, CAMERA_KEYS, CASES, UNSAT_CASES, load_case,
                                translation_residual)
from tests.helpers import load_golden, rel_l2, scene_inputs, settings_for, upstream

pytestmark = pytest.mark.gpu

REF_TOL = 2e-5
IDENTITY_TOL = 1e-6
SELECTIONS = {"default": {}, "no_prezero": dict(bwd_prezero=0), "per_lane": dict(pbwd_lds_sh=0)}


@functools.lru_cache(maxsize=None)
def _fixture():
    return load_golden("camgrad")


@functools.lru_cache(maxsize=None)
def _case(name):
    return load_case(name, _fixture())


def _forward(inp, device, colors_precomp=None, cov3D_precomp=None, antialiasing=False):
    from gaussian_splatting_lightning_amd.rasterizer import forward_raw
    t = lambda a: None if a is None else torch.as_tensor(np.asarray(a, np.float32), device=device)  # noqa: E731
    rs = settings_for(inp, device, antialiasing=antialiasing)
    use_cov = cov3D_precomp is not None
    st = forward_raw(t(inp["means3D"]), None if colors_precomp is not None else t(inp["shs"]), t(colors_precomp),
                     t(inp["opacities"]), None if use_cov else t(inp["scales"]), None if use_cov else t(inp["rotations"]),
                     t(cov3D_precomp), rs)[3]
    return st, rs


def _backward(st, rs, dc, di, **kw):
    from gaussian_splatting_lightning_amd.rasterizer import backward_raw
    t = lambda a: None if a is None else torch.as_tensor(np.asarray(a, np.float32), device=st.means3D.device)  # noqa: E731
    return backward_raw(st, rs, t(dc), t(di), **kw)


def _tiles(st, rs):
    """Kept-tile count of every Gaussian, from the forward's geometry buffer."""
    from gaussian_splatting_lightning_amd import _native
    P = st.means3D.shape[0]
    off = _native.state_layout(P, st.num_rendered, rs.image_width, rs.image_height)["geom_tiles"]
    tiles = st.geom_buffer[off: off + 4 * P].view(torch.int32).cpu().numpy()
    return np.where(st.radii.cpu().numpy() > 0, tiles, 0)


def _assert_structure(g):
    assert tuple(g["viewmatrix"].shape) == (4, 4) and tuple(g["projmatrix"].shape) == (4, 4)
    assert tuple(g["campos"].shape) == (3,)
    assert not g["viewmatrix"][:, 3].any().item(), "column 3 of dL/dviewmatrix is structurally zero"
    assert not g["projmatrix"][:, 2].any().item(), "column 2 of dL/dprojmatrix is structurally zero"


@pytest.mark.parametrize("selection", list(SELECTIONS))
@pytest.mark.parametrize("name", CASES)
def test_reference_parity(gpu_device, name, selection):
    """Relative L2 against the reference's autograd gradients, per tensor; every other gradient bitwise what it is
    without the camera outputs.  big_sh3_208x144 also holds 5 visible Gaussians outside the EWA clamp, whose clamp the
    camera gradients differentiate as the reference does (achieved figures: profiles/camera_grad.json)."""
    from gaussian_splatting_lightning_amd import _native
    inp, dc, di, ref = _case(name)
    with _native.tuned(**SELECTIONS[selection]):
        st, rs = _forward(inp, gpu_device)
        g = _backward(st, rs, dc, di, camera_grads=True)
        plain = _backward(st, rs, dc, di)
    if name == BIG_CASE:
        assert _tiles(st, rs).max() > BIG_GAUSSIAN_TILES, "no Gaussian takes the big-Gaussian path"
    _assert_structure(g)
    err = {k: rel_l2(g[k].cpu().numpy(), ref[k]) for k in CAMERA_KEYS}
    print(name, selection, err)
    parity.record(f"camera_grad[{name}-{selection}]", "reference", err)
    for k in CAMERA_KEYS:
        assert err[k] <= REF_TOL, (k, err[k])
    # every other gradient is bitwise what it is without the camera gradients
    assert set(g) - set(plain) == set(CAMERA_KEYS)
    differ = [k for k, v in plain.items() if (v is None) != (g[k] is None) or (v is not None and not torch.equal(v, g[k]))]
    assert not differ, differ


@pytest.mark.parametrize("name", [UNSAT_CASES[0], BIG_CASE])
def test_deterministic(gpu_device, name):
    inp, dc, di, _ = _case(name)
    st, rs = _forward(inp, gpu_device)
    a = _backward(st, rs, dc, di, camera_grads=True)
    b = _backward(st, rs, dc, di, camera_grads=True)
    for k in CAMERA_KEYS:
        assert torch.equal(a[k], b[k]), k


def _cov3d(inp):
    q = inp["rotations"].astype(np.float64)
    w, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                  2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                  2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    L = R * inp["scales"].astype(np.float64)[:, None, :]
    C = L @ L.transpose(0, 2, 1)
    return np.stack([C[:, 0, 0], C[:, 0, 1], C[:, 0, 2], C[:, 1, 1], C[:, 1, 2], C[:, 2, 2]], 1).astype(np.float32)


def identity_scene(P, W=96, H=80):
    """P Gaussians whose centres all lie inside the EWA Jacobian's 1.3 tan(fov) clamp (or behind the near plane, culled).
    Outside the clamp dL/dmeans3D keeps the upstream CUDA convention (the clamped t.x / t.y taken as constants) while
    the camera gradients differentiate the clamp as written, as the reference does, so the identity -- which needs one
    convention on both sides -- is stated for Gaussians inside it: the first P such of a seeded scene, chosen from
    the inputs alone, in float64 with the limit at 1.29 so that no centre sits at the fp32 edge."""
    inp = scene_inputs(2 * P + 16, W, H, sh_degree=3, seed=20 + P, opacity_scale=0.3, bg=(0.2, 0.5, 0.9))
    t = np.c_[inp["means3D"].astype(np.float64), np.ones(len(inp["means3D"]))] @ inp["viewmatrix"].astype(np.float64)
    z = np.where(t[:, 2] > 0.2, t[:, 2], 1.0)
    keep = (t[:, 2] <= 0.2) | ((np.abs(t[:, 0] / z) <= 1.29 * inp["tanfovx"]) & (np.abs(t[:, 1] / z) <= 1.29 * inp["tanfovy"]))
    idx = np.nonzero(keep)[0][:P]
    assert len(idx) == P
    for k in ("means3D", "opacities", "scales", "rotations", "shs"):
        inp[k] = np.ascontiguousarray(inp[k][idx])
    return inp


def _identity(gpu_device, label, P, invdepth=True, antialiasing=False, colors_precomp=False, cov3D_precomp=False):
    W, H = 96, 80
    inp = identity_scene(P, W, H)
    dc, di = upstream(W, H, P)
    colors = np.random.default_rng(P).random((P, 3), dtype=np.float32) if colors_precomp else None
    st, rs = _forward(inp, gpu_device, colors, _cov3d(inp) if cov3D_precomp else None, antialiasing)
    g = _backward(st, rs, dc, di if invdepth else None, camera_grads=True)
    _assert_structure(g)
    dm = g["means3D"].double().cpu().numpy()
    res, scale = translation_residual(inp["viewmatrix"], inp["projmatrix"], dm.sum(0), g["viewmatrix"].cpu().numpy(),
                                      g["projmatrix"].cpu().numpy(), g["campos"].cpu().numpy(), np.abs(dm).sum(0))
    print(label, "residual", res, "scale", scale)
    parity.record(f"camera_grad[{label}]", "translation_identity",
                  dict(residual=res.tolist(), scale=scale.tolist(),
                       relative=float(np.max(np.abs(res) / np.maximum(scale, 1e-300)))))
    assert scale.min() > 0, "the scene renders nothing: the identity would be empty"
    assert np.all(np.abs(res) <= IDENTITY_TOL * scale), (res, scale)
    return g


@pytest.mark.parametrize("invdepth", [False, True], ids=["color", "color+invdepth"])
@pytest.mark.parametrize("P", [1, 63, 257, 2000])
def test_translation_identity(gpu_device, P, invdepth):
    _identity(gpu_device, f"identity-P{P}-{'inv' if invdepth else 'noinv'}", P, invdepth=invdepth)


def test_translation_identity_antialiasing(gpu_device):
    _identity(gpu_device, "identity-antialiasing", 2000, antialiasing=True)


def test_colors_precomp_has_no_campos_gradient(gpu_device):
    g = _identity(gpu_device, "identity-colors_precomp", 2000, colors_precomp=True)
    assert not g["campos"].any().item()


def test_cov3d_precomp_identity(gpu_device):
    _identity(gpu_device, "identity-cov3D_precomp", 2000, cov3D_precomp=True)


def test_chunked_backward_sums_to_reference(gpu_device):
    from gaussian_splatting_lightning_amd.rasterizer import backward_chunked
    inp, dc, di, ref = _case(UNSAT_CASES[0])
    st, rs = _forward(inp, gpu_device)
    P, M = st.means3D.shape[0], st.M
    assert P > 512
    f32 = dict(dtype=torch.float32, device=gpu_device)
    chunks = []
    for g0, g1 in ((0, 256), (256, 512), (512, P)):
        out = dict(means3D=torch.empty(g1 - g0, 3, **f32), shs=torch.empty(g1 - g0, M, 3, **f32),
                   viewmatrix=torch.full((4, 4), float("nan"), **f32),
                   projmatrix=torch.full((4, 4), float("nan"), **f32), campos=torch.full((3,), float("nan"), **f32))
        chunks.append((g0, g1, out))
    t = lambda a: torch.as_tensor(a, **f32)  # noqa: E731
    backward_chunked(st, rs, t(dc), t(di), chunks)
    whole = _backward(st, rs, dc, di, camera_grads=True)
    err = {}
    for k in CAMERA_KEYS:
        total = sum(out[k].double() for _, _, out in chunks).cpu().numpy()
        err[k] = rel_l2(total, ref[k])
        assert err[k] <= REF_TOL, (k, err[k])
    parity.record("camera_grad[chunked]", "reference", err)
    # the per-Gaussian gradients of the chunks are those of the one-call backward
    assert torch.equal(torch.cat([out["means3D"] for _, _, out in chunks]), whole["means3D"])


def test_autograd_chains_the_three_gradients(gpu_device):
    from gaussian_splatting_lightning_amd.rasterizer import GaussianRasterizationSettings, rasterize_gaussians
    inp, dc, di, _ = _case(UNSAT_CASES[0])
    t = lambda a: torch.as_tensor(np.asarray(a, np.float32), device=gpu_device)  # noqa: E731
    dc, di = t(dc), t(di)
    V0 = t(inp["viewmatrix"])
    Pj = torch.linalg.inv(V0.double()) @ t(inp["projmatrix"]).double()  # projmatrix = V @ Pj
    Pj = Pj.to(torch.float32)
    scene = [t(inp[k]) for k in ("means3D", "shs", "opacities", "scales", "rotations")]

    def render(V, proj, campos, leaves):
        rs = GaussianRasterizationSettings(
            image_height=inp["image_height"], image_width=inp["image_width"], tanfovx=inp["tanfovx"],
            tanfovy=inp["tanfovy"], bg=t(inp["bg"]), scale_modifier=inp["scale_modifier"], viewmatrix=V,
            projmatrix=proj, sh_degree=inp["sh_degree"], campos=campos, prefiltered=False, debug=False,
            antialiasing=False)
        means, shs, opac, sc, rot = leaves
        img, _radii, invd = rasterize_gaussians(means, torch.zeros_like(means), shs, None, opac, sc, rot, None, rs)
        return img, (img * dc).sum() + (invd * di).sum()

    def camera(V):
        return V @ Pj, torch.linalg.inv(V)[3, :3]

    # pose optimisation: V a leaf, projmatrix and campos built from it in torch
    V = V0.clone().requires_grad_(True)
    leaves = [x.clone().requires_grad_(True) for x in scene]
    img, loss = render(V, *camera(V), leaves)
    loss.backward()
    assert V.grad is not None and tuple(V.grad.shape) == (4, 4)
    # the same chain by hand from the three raw gradients, on detached copies
    Vd = V0.clone().requires_grad_(True)
    proj_d, campos_d = camera(Vd)
    from gaussian_splatting_lightning_amd.rasterizer import backward_raw, forward_raw
    rs2 = settings_for(inp, gpu_device)._replace(viewmatrix=Vd.detach(), projmatrix=proj_d.detach(),
                                                 campos=campos_d.detach())
    st2 = forward_raw(scene[0], scene[1], None, scene[2], scene[3], scene[4], None, rs2)[3]
    raw = backward_raw(st2, rs2, dc, di, camera_grads=True)
    (chain,) = torch.autograd.grad([proj_d, campos_d], [Vd], [raw["projmatrix"], raw["campos"]])
    chain = chain + raw["viewmatrix"]
    err = rel_l2(V.grad.cpu().numpy(), chain.cpu().numpy())
    print("autograd chain", err)
    parity.record("camera_grad[autograd]", "chain", dict(viewmatrix=err))
    assert err <= 1e-6  # the same three tensors through the same two torch ops: fp32 rounding of one 4x4 chain

    # no camera tensor requiring grad: image and gradients bitwise those of a call with detached camera tensors
    leaves_a = [x.clone().requires_grad_(True) for x in scene]
    leaves_b = [x.clone().requires_grad_(True) for x in scene]
    img_a, loss_a = render(V0, *camera(V0), leaves_a)
    Vn = V0.clone().requires_grad_(True)
    pn, cn = camera(Vn)
    img_b, loss_b = render(Vn.detach(), pn.detach(), cn.detach(), leaves_b)
    loss_a.backward()
    loss_b.backward()
    assert Vn.grad is None
    assert torch.equal(img_a, img_b) and torch.equal(img_a, img.detach())
    for a, b, c in zip(leaves_a, leaves_b, leaves):
        assert torch.equal(a.grad, b.grad) and torch.equal(a.grad, c.grad)


def test_no_gaussians_gives_zero_camera_gradients(gpu_device):
    """P == 0 (gsr_backward's early return): the three outputs are zeroed, on the caller's stream."""
    import ctypes

    from gaussian_splatting_lightning_amd import _native
    lib = _native.load()
    out = [torch.full((n,), float("nan"), dtype=torch.float32, device=gpu_device) for n in (16, 16, 3)]
    a = _native.BackwardArgs(P=0, W=96, H=80, dL_dviewmatrix=out[0].data_ptr(), dL_dprojmatrix=out[1].data_ptr(),
                             dL_dcampos=out[2].data_ptr())
    cb = _native.ALLOC_FN(lambda c, w, b: None)
    with torch.cuda.device(gpu_device):
        rc = lib.gsr_backward(ctypes.byref(a), cb, None, torch.cuda.current_stream(gpu_device).cuda_stream)
    _native.check(rc, "gsr_backward")
    for t in out:
        assert not t.any().item() and not torch.isnan(t).any().item()
