"""Per-Gaussian feature channels (gsr_forward_features / gsr_backward_features, forward_raw(features=...),
backward_raw(grad_out_features=...), rasterize_gaussians(features=...)) on the GPU.

Truth: tests/feature_cases.py -- the CPU oracle alone, by linearity: one precomputed-colour run per chunk of three
channels, the chunks' geometry gradients summed in float64, the SH colour run (and scene A's alpha gradient and
background image, composed as tests/test_alpha_background.py does) added for the joint call.  The scenes are those of
tests/absgrad_cases.py: no threshold-flip candidate in any of them, asserted from the oracle with every truth, so the
bars are the project's clean bars (COLOR_TOL, GRAD_CLEAN_TOL) without a flip term and no pixel or Gaussian is left out
of a comparison.  Achieved figures: profiles/parity_features.json.
"""
import numpy as np
import pytest
import torch

from tests import absgrad_cases as AC
from tests import feature_cases as F
from tests import parity
from tests import test_alpha_background as TAB
from tests.helpers import rel_l2, settings_for
from tests.test_absgrad import SELECTIONS
from tests.test_gpu_parity import COLOR_TOL, GRAD_CLEAN_TOL, GRAD_TOL_ADHOC

pytestmark = pytest.mark.gpu

f32 = np.float32
SCENES = ("A", "A2", "B")
CAMERA_TOL = 2e-5  # the README's camera-gradient bar
# every forward-form knob set of tests/test_alpha_background.py::test_every_forward_form_writes_alpha_and_the_image
FORWARD_FORMS = next(m for m in TAB.test_every_forward_form_writes_alpha_and_the_image.pytestmark
                     if m.name == "parametrize").args[1]
GRAD_NAMES = F.GEOMETRY + ("shs",)


def _t(a, dev):
    return None if a is None else torch.as_tensor(np.asarray(a, f32), device=dev)


def _forward(inp, dev, features=None, colors=None, bg=None, return_alpha=False):
    """forward_raw on the scene: SH colours unless `colors` (P,3) is given.  Returns (settings, result tuple)."""
    from gaussian_splatting_lightning_amd.rasterizer import forward_raw
    rs = settings_for(inp, dev)
    if bg is not None:
        rs = rs._replace(bg=_t(bg, dev))
    kw = {} if features is None else dict(features=features if torch.is_tensor(features) else _t(features, dev))
    res = forward_raw(_t(inp["means3D"], dev), None if colors is not None else _t(inp["shs"], dev), _t(colors, dev),
                      _t(inp["opacities"], dev), _t(inp["scales"], dev), _t(inp["rotations"], dev), None, rs,
                      return_alpha=return_alpha, **kw)
    return rs, res


def _run(inp, dev, features=None, dc=None, di=None, dF=None, knobs=None, bg=None, colors=None, **kw):
    """Forward + backward_raw under the knobs; returns (gradients on the device, feature image or None)."""
    from gaussian_splatting_lightning_amd import _native
    from gaussian_splatting_lightning_amd.rasterizer import backward_raw
    with _native.tuned(**(knobs or {})):
        rs, res = _forward(inp, dev, features, colors=colors, bg=bg)
        if dF is not None:
            kw["grad_out_features"] = _t(dF, dev)
        g = backward_raw(res[-1], rs, _t(dc, dev), _t(di, dev), **kw)
        torch.cuda.synchronize()
    g["radii"] = res[1]
    return g, (res[3] if features is not None else None)


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------ 1. forward parity
@pytest.mark.parametrize("C", [1, 3, 7, 33, 64])
@pytest.mark.parametrize("name", SCENES)
def test_forward_parity(gpu_device, name, C):
    inp = F.scene(name)[0]
    f, _ = F.inputs(name, C)
    t = F.truth(name, C)
    assert t["flip_candidates"] == 0
    n, W, H = AC.SCENES[name][:3]
    _, (color, radii, invd, image, st) = _forward(inp, gpu_device, f)
    assert image.shape == (C, H, W) and image.dtype == torch.float32 and st.features.shape == (n, C)
    got = image.cpu().numpy()
    err = np.abs(got - t["image"]) / np.maximum(1.0, np.abs(t["image"]))
    rec = dict(maxrel=float(err.max()), bar=COLOR_TOL, pixels=int(W * H), nonzero_pixels=int((t["image"][0] != 0).sum()))
    parity.record(f"features_forward_{name}_C{C}", "image_vs_oracle", rec)
    print(name, C, rec)
    assert rec["maxrel"] <= COLOR_TOL, rec  # every pixel
    assert np.all(got[:, t["image"][0] == 0] == 0)  # where no Gaussian reaches: exact zeros, no background term
    # colour, radii and inverse depth are those of the call without features
    _, (c0, r0, i0, _) = _forward(inp, gpu_device)
    assert _bits(color, c0) and torch.equal(radii, r0) and _bits(invd, i0)
    if C == 3:  # the same values as colours over a zero background: the same sum in the same order
        _, (c3, _, _, _) = _forward(inp, gpu_device, colors=f, bg=np.zeros(3, f32))
        assert _bits(image, c3)


# ------------------------------------------------------------------------------------------------ 2. forward forms
@pytest.mark.parametrize("knobs", FORWARD_FORMS, ids=lambda k: "-".join(f"{n}{v}" for n, v in k.items()))
def test_every_forward_form_gives_the_same_feature_image(gpu_device, knobs):
    from gaussian_splatting_lightning_amd import _native
    for name, C in (("A", 7), ("B", 33)):
        inp = F.scene(name)[0]
        f, _ = F.inputs(name, C)
        assert F.truth(name, C)["flip_candidates"] == 0
        _, (_, _, _, _, image_def, _) = _forward(inp, gpu_device, f, return_alpha=True)
        with _native.tuned(**knobs):
            _, (color, radii, invd, alpha, image, _) = _forward(inp, gpu_device, f, return_alpha=True)
            _, (c0, r0, i0, a0, _) = _forward(inp, gpu_device, return_alpha=True)
        assert _bits(image, image_def), name  # the replay reads only recorded state
        assert _bits(color, c0) and torch.equal(radii, r0) and _bits(invd, i0) and _bits(alpha, a0), name


# ------------------------------------------------------------------------------------------------ 3. backward parity
def _compare(case, got, truth, names):
    rec = {k: dict(rel_l2=rel_l2(got[k].cpu().numpy().reshape(np.shape(truth[k])), truth[k]), bar=GRAD_CLEAN_TOL)
           for k in names}
    parity.record(case, "backward", rec)
    print(case, {k: v["rel_l2"] for k, v in rec.items()})
    for k in names:
        assert rec[k]["rel_l2"] <= GRAD_CLEAN_TOL, (case, k, rec[k])


@pytest.mark.parametrize("selection", list(SELECTIONS))
@pytest.mark.parametrize("C", [1, 7, 33])
@pytest.mark.parametrize("name", SCENES)
def test_backward_parity_features_alone(gpu_device, name, C, selection):
    """Every gradient comes from the features (the colour's upstream gradient is zero): the live-flag case."""
    inp = F.scene(name)[0]
    f, dF = F.inputs(name, C)
    t = F.truth(name, C)
    assert t["flip_candidates"] == 0
    g, _ = _run(inp, gpu_device, f, dF=dF, knobs=SELECTIONS[selection])
    assert g["features"].shape == f.shape and g["features"].dtype == torch.float32
    _compare(f"features_alone_{name}_C{C}_{selection}", g, t, ("features",) + F.GEOMETRY)
    # the Gaussians with a non-zero gradient are the oracle's: none dropped by the live flags, none invented
    for k in ("features", "opacities", "means3D", "means2D"):
        got_nz = (g[k].reshape(len(f), -1) != 0).any(1).cpu().numpy()
        want_nz = (np.asarray(t[k]).reshape(len(f), -1) != 0).any(1)
        assert np.array_equal(got_nz, want_nz), (k, int(got_nz.sum()), int(want_nz.sum()))
    assert float(g["shs"].abs().max()) == 0.0
    assert torch.all(g["features"][g["radii"] == 0] == 0)


@pytest.mark.parametrize("selection", list(SELECTIONS))
@pytest.mark.parametrize("C", [1, 7, 33])
@pytest.mark.parametrize("name", SCENES)
def test_backward_parity_joint(gpu_device, name, C, selection):
    """SH colour + inverse depth + features in one call; on scene A also with an alpha gradient and a (3,H,W)
    background."""
    inp, dc, di = F.scene(name)
    f, dF = F.inputs(name, C)
    t = F.joint_truth(name, C)
    assert t["flip_candidates"] == 0
    g, _ = _run(inp, gpu_device, f, dc, di, dF, knobs=SELECTIONS[selection])
    _compare(f"features_joint_{name}_C{C}_{selection}", g, t, ("features",) + GRAD_NAMES)
    if name == "A":
        da, image = AC.ext_inputs()
        t = F.joint_truth(name, C, ext=True)
        assert t["flip_candidates"] == 0
        g, _ = _run(inp, gpu_device, f, dc, di, dF, knobs=SELECTIONS[selection], bg=image,
                    grad_out_alpha=_t(da, gpu_device))
        _compare(f"features_joint_ext_{name}_C{C}_{selection}", g, t, ("features",) + GRAD_NAMES)


# ------------------------------------------------------------------------------------------------ 4. camera gradients
def test_camera_gradients_of_the_joint_call(gpu_device):
    """Against the sum of the GPU's own chunked 3-channel colors_precomp calls plus the colour call."""
    inp, dc, di = F.scene("A")
    C = 7
    f, dF = F.inputs("A", C)
    names = ("viewmatrix", "projmatrix", "campos")
    g, _ = _run(inp, gpu_device, f, dc, di, dF, camera_grads=True)
    want = {k: v.double() for k, v in _run(inp, gpu_device, None, dc, di, camera_grads=True)[0].items() if k in names}
    for c0 in range(0, C, 3):
        w = min(3, C - c0)
        part, _ = _run(inp, gpu_device, None, np.pad(dF[c0:c0 + w], ((0, 3 - w), (0, 0), (0, 0))), None,
                       colors=np.pad(f[:, c0:c0 + w], ((0, 0), (0, 3 - w))), bg=np.zeros(3, f32), camera_grads=True)
        for k in names:
            want[k] = want[k] + part[k].double()
    rec = {k: dict(rel_l2=rel_l2(g[k].cpu().numpy(), want[k].cpu().numpy()), bar=CAMERA_TOL) for k in names}
    parity.record("features_camera_A_C7", "camera_vs_chunked_calls", rec)
    print(rec)
    for k in names:
        assert rec[k]["rel_l2"] <= CAMERA_TOL, (k, rec[k])
    assert float(want["viewmatrix"].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 5. neutrality
@pytest.mark.parametrize("name", ["A", "B"])
def test_no_feature_gradient_keeps_every_bit(gpu_device, name):
    inp, dc, di = F.scene(name)
    f, _ = F.inputs(name, 7)
    plain, _ = _run(inp, gpu_device, None, dc, di, camera_grads=True)
    g, _ = _run(inp, gpu_device, f, dc, di, None, camera_grads=True)
    for k in GRAD_NAMES + ("viewmatrix", "projmatrix", "campos"):
        assert _bits(g[k], plain[k]), k
    assert g["features"].shape == f.shape and torch.all(g["features"] == 0) and "features" not in plain


@pytest.mark.parametrize("name,C", [("A", 7), ("A2", 33), ("B", 16)])
def test_calls_repeat_bit_for_bit(gpu_device, name, C):
    inp, dc, di = F.scene(name)
    f, dF = F.inputs(name, C)
    a, ia = _run(inp, gpu_device, f, dc, di, dF, camera_grads=True)
    b, ib = _run(inp, gpu_device, f, dc, di, dF, camera_grads=True)
    assert _bits(ia, ib)
    for k in ("features",) + GRAD_NAMES + ("viewmatrix", "projmatrix", "campos"):
        assert not torch.isnan(a[k]).any() and _bits(a[k], b[k]), k


@pytest.mark.parametrize("name", ["A", "B"])
def test_unaligned_features_and_nan_prefilled_outputs(gpu_device, name):
    """C = 7 rows are 28 B: with the tensor a view 4 B off a 16-B boundary no row is 16-B aligned; the outputs are
    NaN-prefilled.  The same bits as aligned fresh ones, under bwd_prezero / bwd_live 0 and 1."""
    inp, dc, di = F.scene(name)
    C, P = 7, AC.SCENES[name][0]
    f, dF = F.inputs(name, C)
    want, image = _run(inp, gpu_device, f, dc, di, dF)
    buf = torch.zeros(P * C + 8, device=gpu_device)
    assert buf.data_ptr() % 16 == 0
    view = buf[1:1 + P * C].view(P, C)
    view.copy_(_t(f, gpu_device))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    for prezero, live in ((1, 1), (0, 1), (1, 0), (0, 0)):
        obuf = torch.full((P * C + 8,), float("nan"), device=gpu_device)
        out = {"features": obuf[1:1 + P * C].view(P, C), "means3D": torch.full((P, 3), float("nan"), device=gpu_device),
               "opacities": torch.full((P, 1), float("nan"), device=gpu_device)}
        got, image2 = _run(inp, gpu_device, view, dc, di, dF, knobs=dict(bwd_prezero=prezero, bwd_live=live), out=out)
        assert got["features"].data_ptr() == out["features"].data_ptr() and _bits(image, image2)
        assert _bits(got["features"], want["features"]), (prezero, live)
        for k in GRAD_NAMES:  # (up to the sign of a zero: the zero fill's +0 or the per-Gaussian arithmetic's -0)
            assert not torch.isnan(got[k]).any() and torch.equal(got[k], want[k]), (k, prezero, live)
        assert torch.isnan(obuf[0]) and torch.isnan(obuf[1 + P * C:]).all()  # nothing written around it


# ------------------------------------------------------------------------------------------------ 6. autograd
def test_autograd_surface(gpu_device):
    from gaussian_splatting_lightning_amd import GaussianRasterizer
    inp, dc, di = F.scene("A")
    dev = gpu_device
    C = 7
    f, dF = F.inputs("A", C)
    n, W, H = AC.SCENES["A"][:3]

    def leaves():
        lv = {k: _t(inp[k], dev).requires_grad_(True) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
        lv["features"] = _t(f, dev).requires_grad_(True)
        lv["means2D"] = torch.zeros(n, 3, device=dev, requires_grad=True)
        return lv

    def call(rast, lv, **kw):
        return rast(means3D=lv["means3D"], means2D=lv["means2D"], opacities=lv["opacities"], shs=lv["shs"],
                    scales=lv["scales"], rotations=lv["rotations"], **kw)

    # five outputs in the documented order; without features the call is what it was
    lv = leaves()
    out = call(GaussianRasterizer(settings_for(inp, dev), return_alpha=True), lv, features=lv["features"])
    assert len(out) == 5
    color, radii, invd, alpha, image = out
    assert color.shape == (3, H, W) and radii.shape == (n,) and invd.shape == (1, H, W) and alpha.shape == (1, H, W)
    assert image.shape == (C, H, W) and image.requires_grad
    assert len(call(GaussianRasterizer(settings_for(inp, dev), return_alpha=True), leaves())) == 4
    assert len(call(GaussianRasterizer(settings_for(inp, dev)), leaves())) == 3
    # a loss on the feature image alone
    (image * _t(dF, dev)).sum().backward()
    raw, _ = _run(inp, dev, f, dF=dF)
    assert lv["features"].grad is not None and float(lv["features"].grad.abs().max()) > 0
    assert float(lv["means3D"].grad.abs().max()) > 0
    rec = {}
    for k, r in (("features", "features"), ("means3D", "means3D"), ("means2D", "means2D"), ("opacities", "opacities"),
                 ("scales", "scales"), ("rotations", "rotations")):
        rec[k] = rel_l2(lv[k].grad.cpu().numpy(), raw[r].cpu().numpy().reshape(lv[k].grad.shape))
    # the joint loss through the four-output form
    lv = leaves()
    color, radii, invd, image = call(GaussianRasterizer(settings_for(inp, dev)), lv, features=lv["features"])
    ((color * _t(dc, dev)).sum() + (invd * _t(di, dev)).sum() + (image * _t(dF, dev)).sum()).backward()
    raw, _ = _run(inp, dev, f, dc, di, dF)
    for k in ("features", "means3D", "shs", "opacities"):
        rec["joint_" + k] = rel_l2(lv[k].grad.cpu().numpy(), raw[k].cpu().numpy().reshape(lv[k].grad.shape))
    parity.record("features_autograd_A_C7", "autograd_vs_backward_raw", dict(rec, bar=GRAD_TOL_ADHOC))
    print(rec)
    for k, v in rec.items():
        assert v <= GRAD_TOL_ADHOC, (k, v)


# ------------------------------------------------------------------------------------------------ 7. empty scenes
def test_empty_scenes(gpu_device):
    from gaussian_splatting_lightning_amd.rasterizer import backward_raw, forward_raw
    inp, dc, di = F.scene("A")
    dev = gpu_device
    n, W, H = AC.SCENES["A"][:3]
    f, dF = F.inputs("A", 5)
    rs = settings_for(inp, dev)
    e = lambda *s: torch.zeros(0, *s, device=dev)  # noqa: E731
    color, radii, invd, image, st = forward_raw(e(3), e(16, 3), None, e(1), e(3), e(4), None, rs, features=e(5))
    g = backward_raw(st, rs, _t(dc, dev), _t(di, dev), grad_out_features=_t(dF, dev))
    torch.cuda.synchronize()
    assert image.shape == (5, H, W) and torch.all(image == 0) and g["features"].shape == (0, 5)
    # every Gaussian behind the camera: nothing rendered, zeros (the gradient's destination is NaN-prefilled)
    ph = np.asarray([0.0, 0.0, -1.0, 1.0]) @ np.linalg.inv(inp["viewmatrix"].astype(np.float64))
    behind = dict(inp, means3D=(inp["means3D"] * f32(0.01) + (ph[:3] / ph[3]).astype(f32)).astype(f32))
    out = {"features": torch.full((n, 5), float("nan"), device=dev)}
    g, image = _run(behind, dev, f, dc, di, dF, out=out)
    assert torch.all(g["radii"] == 0) and torch.all(image == 0)
    assert torch.all(g["features"] == 0) and torch.all(g["means3D"] == 0)


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_on_the_device_path(gpu_device):
    from gaussian_splatting_lightning_amd import GaussianRasterizer
    from gaussian_splatting_lightning_amd.rasterizer import backward_chunked, backward_raw
    inp, dc, di = F.scene("A")
    dev = gpu_device
    f, dF = F.inputs("A", 4)
    rs, res = _forward(inp, dev, f)
    st = res[-1]
    with pytest.raises(NotImplementedError):
        backward_raw(st, rs, _t(dc, dev), _t(di, dev), grad_out_features=_t(dF, dev), absgrad=True)
    with pytest.raises(NotImplementedError):
        backward_chunked(st, rs, _t(dc, dev), _t(di, dev), [(0, len(f), {})])
    with pytest.raises(NotImplementedError):
        GaussianRasterizer(rs, absgrad=True)(means3D=_t(inp["means3D"], dev), means2D=None,
                                             opacities=_t(inp["opacities"], dev), shs=_t(inp["shs"], dev),
                                             scales=_t(inp["scales"], dev), rotations=_t(inp["rotations"], dev),
                                             features=_t(f, dev))
    # the state still serves a plain backward afterwards
    g = backward_raw(st, rs, _t(dc, dev), _t(di, dev), grad_out_features=_t(dF, dev))
    torch.cuda.synchronize()
    assert float(g["features"].abs().max()) > 0
