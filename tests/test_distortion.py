"""The depth distortion map (gsr_forward_distortion / gsr_backward_distortion, forward_raw(distortion=...),
backward_raw(grad_out_distortion=...), rasterize_gaussians(distortion=...)) on the GPU.

Truth: tests/distortion_cases.py through tests/golden/distortion.npz -- the CPU oracle alone: its per-pixel weights,
D, dD/dw and dD/dt in float64, the gradient through the weights from oracle runs with the frozen dD/dw as precomputed
colours, the depth part analytically.  The scenes are those of tests/absgrad_cases.py: no threshold-flip candidate in
any of them, asserted with every truth, so no pixel and no Gaussian is left out of a comparison.

Bars (distortion_cases.bar): the larger of the suite's clean bar (COLOR_TOL, GRAD_CLEAN_TOL: the oracle part of the
truth carries the suite's fp32 error) and 4 x the error of the worse of two numpy float32 restatements of the formulas
against the float64 truth -- what the distortion's own cancellation costs in fp32, measured by the generator and
stored in the fixture, never taken from the device's output.  Achieved figures: profiles/parity_distortion.json.
"""
import numpy as np
import pytest
import torch

from tests import absgrad_cases as AC
from tests import distortion_cases as DC
from tests import feature_cases as F
from tests import parity
from tests import test_alpha_background as TAB
from tests.helpers import rel_l2, settings_for
from tests.test_absgrad import SELECTIONS
from tests.test_gpu_parity import COLOR_TOL, GRAD_CLEAN_TOL, GRAD_TOL_ADHOC

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
CAMERA_TOL = 2e-5  # the README's camera-gradient bar
# every forward-form knob set of tests/test_alpha_background.py::test_every_forward_form_writes_alpha_and_the_image
FORWARD_FORMS = next(m for m in TAB.test_every_forward_form_writes_alpha_and_the_image.pytestmark
                     if m.name == "parametrize").args[1]
GRAD_NAMES = DC.GEOMETRY + ("shs",)
CAMERA = ("viewmatrix", "projmatrix", "campos")
C_FEAT = 7


def _t(a, dev):
    return None if a is None else torch.as_tensor(np.asarray(a, f32), device=dev)


def _dist_kw(which):
    return {} if which is None else dict(distortion=which, distortion_near=DC.NEAR, distortion_far=DC.FAR)


def _forward(inp, dev, which=None, features=None, colors=None, bg=None, return_alpha=False):
    """forward_raw on the scene: SH colours unless `colors` (P,3) is given.  Returns (settings, result tuple)."""
    from gaussian_splatting_lightning_amd.rasterizer import forward_raw
    rs = settings_for(inp, dev)
    if bg is not None:
        rs = rs._replace(bg=_t(bg, dev))
    kw = dict(_dist_kw(which), **({} if features is None else dict(features=_t(features, dev))))
    res = forward_raw(_t(inp["means3D"], dev), None if colors is not None else _t(inp["shs"], dev), _t(colors, dev),
                      _t(inp["opacities"], dev), _t(inp["scales"], dev), _t(inp["rotations"], dev), None, rs,
                      return_alpha=return_alpha, **kw)
    return rs, res


def _run(inp, dev, which=None, dc=None, di=None, gD=None, features=None, dF=None, knobs=None, colors=None, bg=None,
         **kw):
    """Forward + backward_raw under the knobs; returns (gradients on the device, distortion map or None)."""
    from gaussian_splatting_lightning_amd import _native
    from gaussian_splatting_lightning_amd.rasterizer import backward_raw
    with _native.tuned(**(knobs or {})):
        rs, res = _forward(inp, dev, which, features, colors=colors, bg=bg)
        if gD is not None:
            kw["grad_out_distortion"] = _t(gD, dev)
        if dF is not None:
            kw["grad_out_features"] = _t(dF, dev)
        g = backward_raw(res[-1], rs, _t(dc, dev), _t(di, dev), **kw)
        torch.cuda.synchronize()
    g["radii"] = res[1]
    return g, (res[-2] if which is not None else None)


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _truth(name, which):
    t = DC.fixture_truth(name, which)
    assert int(t["flip_candidates"]) == 0
    return t


# ------------------------------------------------------------------------------------------------ 1. forward parity
@pytest.mark.parametrize("which", DC.MAPS)
@pytest.mark.parametrize("name", DC.SCENES)
def test_forward_parity(gpu_device, name, which):
    inp = DC.scene(name)
    t = _truth(name, which)
    n, W, H = AC.SCENES[name][:3]
    _, (color, radii, invd, alpha, D, st) = _forward(inp, gpu_device, which, return_alpha=True)
    assert D.shape == (1, H, W) and D.dtype == torch.float32
    assert st.distortion.map == which and st.distortion.totals.shape == (2, H, W)
    got = D[0].cpu().numpy()
    bar = DC.bar(t, "D", COLOR_TOL)
    rec = dict(maxrel=DC.fwd_error(got, t["D"]), bar=bar, restatement=DC.restatement_error(t, "D"), pixels=int(W * H),
               nonzero_pixels=int((t["D"] != 0).sum()), max_D=float(t["D"].max()))
    parity.record(f"distortion_forward_{name}_{which}", "map_vs_oracle", rec)
    print(name, which, rec)
    assert rec["maxrel"] <= bar, rec  # every pixel
    # exact 0 where no Gaussian reaches (alpha is exactly 0 there)
    untouched = (alpha[0] == 0).cpu().numpy()
    assert untouched.any() or name != "A"  # (scene A leaves 12 pixels untouched; the others cover every pixel)
    assert np.all(got[untouched] == 0) and np.all(t["D"][untouched] == 0)
    # colour, radii, inverse depth and alpha are those of the call without distortion
    _, (c0, r0, i0, a0, _) = _forward(inp, gpu_device, return_alpha=True)
    assert _bits(color, c0) and torch.equal(radii, r0) and _bits(invd, i0) and _bits(alpha, a0)


# ------------------------------------------------------------------------------------------------ 2. forward forms
@pytest.mark.parametrize("knobs", list(FORWARD_FORMS) + [dict(guard=1)],
                         ids=lambda k: "-".join(f"{n}{v}" for n, v in k.items()))
def test_every_forward_form_gives_the_same_map(gpu_device, knobs):
    from gaussian_splatting_lightning_amd import _native
    for name, which in (("A", "z"), ("B", "ndc")):
        inp = DC.scene(name)
        _truth(name, which)  # (no flip candidate: the guarded decision is the plain one on every pair)
        D_def = _forward(inp, gpu_device, which)[1][-2]
        with _native.tuned(**knobs):
            D = _forward(inp, gpu_device, which)[1][-2]
        assert _bits(D, D_def), name  # the replay reads only recorded state


# ------------------------------------------------------------------------------------------------ 3. backward parity
def _compare(case, got, truth, t, names):
    """Relative L2 per tensor against `truth`; the bar from the fixture's restatement errors of (scene, map) `t`."""
    rec = {}
    for k in names:
        norm = float(np.linalg.norm(truth[k]))
        bar = DC.bar(t, k, GRAD_CLEAN_TOL, norm) if k in DC.GEOMETRY else GRAD_CLEAN_TOL
        rec[k] = dict(rel_l2=rel_l2(got[k].cpu().numpy().reshape(np.shape(truth[k])), truth[k]), bar=bar)
    parity.record(case, "backward", rec)
    print(case, {k: (v["rel_l2"], v["bar"]) for k, v in rec.items()})
    for k in names:
        assert rec[k]["rel_l2"] <= rec[k]["bar"], (case, k, rec[k])


@pytest.mark.parametrize("selection", list(SELECTIONS))
@pytest.mark.parametrize("which", DC.MAPS)
@pytest.mark.parametrize("name", DC.SCENES)
def test_backward_parity_distortion_alone(gpu_device, name, which, selection):
    """Every gradient comes from the distortion map (the colour's upstream gradient is zero): the live-flag case."""
    inp = DC.scene(name)
    t = _truth(name, which)
    n = AC.SCENES[name][0]
    g, _ = _run(inp, gpu_device, which, gD=DC.upstream(name), knobs=SELECTIONS[selection])
    _compare(f"distortion_alone_{name}_{which}_{selection}", g, t, t, DC.GEOMETRY)
    # the Gaussians with a non-zero gradient are exactly the truth's: none dropped by the live flags, none invented
    for k in ("opacities", "means3D", "means2D"):
        got_nz = (g[k].reshape(n, -1) != 0).any(1).cpu().numpy()
        want_nz = (np.asarray(t[k]).reshape(n, -1) != 0).any(1)
        assert np.array_equal(got_nz, want_nz), (k, int(got_nz.sum()), int(want_nz.sum()))
    assert float(g["shs"].abs().max()) == 0.0


@pytest.mark.parametrize("selection", list(SELECTIONS))
@pytest.mark.parametrize("which", DC.MAPS)
@pytest.mark.parametrize("name", DC.SCENES)
def test_backward_parity_joint_with_colour(gpu_device, name, which, selection):
    """SH colour + inverse depth + distortion in one call."""
    inp, dc, di = F.scene(name)
    t = _truth(name, which)
    from tests.helpers import run_oracle
    run = run_oracle(dict(inp, bg=np.zeros(3, f32)))[3]
    assert int((run.threshold_margin() < AC.FLIP_MARGIN).sum()) == 0
    a = run.backward(dc, di)
    truth = {k: t[k] + a[k].astype(f64) for k in DC.GEOMETRY}
    truth["shs"] = a["shs"].astype(f64)
    g, _ = _run(inp, gpu_device, which, dc, di, DC.upstream(name), knobs=SELECTIONS[selection])
    _compare(f"distortion_joint_{name}_{which}_{selection}", g, truth, t, GRAD_NAMES)


@pytest.mark.parametrize("selection", list(SELECTIONS))
@pytest.mark.parametrize("which", DC.MAPS)
@pytest.mark.parametrize("name", DC.SCENES)
def test_backward_parity_joint_with_features(gpu_device, name, which, selection):
    """SH colour + inverse depth + features (C = 7) + distortion in one call: the training call."""
    inp, dc, di = F.scene(name)
    f, dF = F.inputs(name, C_FEAT)
    t = _truth(name, which)
    ft = F.joint_truth(name, C_FEAT)
    assert ft["flip_candidates"] == 0
    truth = dict(ft, **{k: ft[k] + t[k] for k in DC.GEOMETRY})
    g, _ = _run(inp, gpu_device, which, dc, di, DC.upstream(name), features=f, dF=dF, knobs=SELECTIONS[selection])
    _compare(f"distortion_features_{name}_{which}_{selection}", g, truth, t, ("features",) + GRAD_NAMES)


# ------------------------------------------------------------------------------------------------ 4. camera gradients
@pytest.mark.parametrize("which", DC.MAPS)
def test_camera_gradients_of_the_joint_call(gpu_device, which):
    """The camera gradients of SH colour + inverse depth + distortion on scene A.  No reference computes this loss, so
    the truth is the chain rule on the truth's terms (the second of the two forms): through the weights, the sum of
    the GPU's own colors_precomp calls with the truth's frozen dD/dw as colours, three pixels a call, whose camera
    gradients tests/test_camera_grad.py holds to the reference; through the depths, analytically from the truth's
    per-Gaussian depth gradient, z = means3D . V[:3,2] + V[3,2]: dV[r][2] += sum_i means3D[i][r] dz_i, dV[3][2] +=
    sum_i dz_i; plus the colour call's own camera gradients."""
    name = "A"
    inp, dc, di = F.scene(name)
    n, W, H = AC.SCENES[name][:3]
    t = _truth(name, which)
    gD = DC.upstream(name)
    g, _ = _run(inp, gpu_device, which, dc, di, gD, camera_grads=True)
    want = {k: v.double().cpu().numpy() for k, v in _run(inp, gpu_device, None, dc, di, camera_grads=True)[0].items()
            if k in CAMERA}
    _, C, _ = DC.coefficients(name, which)
    zero_bg = np.zeros(3, f32)
    for p0 in range(0, W * H, 3):
        col, up = np.zeros((n, 3), f32), np.zeros((3, H, W), f32)
        for ch, pix in enumerate(range(p0, min(p0 + 3, W * H))):
            col[:, ch] = C[pix]
            up[ch, pix // W, pix % W] = gD[0, pix // W, pix % W]
        if not col.any():
            continue
        part, _ = _run(inp, gpu_device, None, up, None, colors=col, bg=zero_bg, camera_grads=True)
        for k in CAMERA:
            want[k] = want[k] + part[k].double().cpu().numpy()
    want["viewmatrix"][:3, 2] += (inp["means3D"].astype(f64) * t["dz"][:, None]).sum(0)
    want["viewmatrix"][3, 2] += t["dz"].sum()
    rec = {k: dict(rel_l2=rel_l2(g[k].cpu().numpy(), want[k]), bar=CAMERA_TOL) for k in CAMERA}
    parity.record(f"distortion_camera_A_{which}", "camera_vs_chain_rule", rec)
    print(rec)
    for k in CAMERA:
        assert rec[k]["rel_l2"] <= CAMERA_TOL, (k, rec[k])
    assert float(np.abs(want["viewmatrix"]).max()) > 0 and float(np.abs(t["dz"]).max()) > 0


# ------------------------------------------------------------------------------------------------ 5. neutrality
@pytest.mark.parametrize("name", ["A", "B"])
def test_no_distortion_gradient_keeps_every_bit(gpu_device, name):
    inp, dc, di = F.scene(name)
    plain, _ = _run(inp, gpu_device, None, dc, di, camera_grads=True)
    g, _ = _run(inp, gpu_device, "ndc", dc, di, None, camera_grads=True)
    for k in GRAD_NAMES + CAMERA:
        assert _bits(g[k], plain[k]), k


# ------------------------------------------------------------------------------------------------ 6. determinism
@pytest.mark.parametrize("name,which", [("A", "z"), ("A2", "ndc"), ("B", "z")])
def test_calls_repeat_bit_for_bit(gpu_device, name, which):
    inp, dc, di = F.scene(name)
    f, dF = F.inputs(name, C_FEAT)
    gD = DC.upstream(name)
    a, Da = _run(inp, gpu_device, which, dc, di, gD, features=f, dF=dF, camera_grads=True)
    b, Db = _run(inp, gpu_device, which, dc, di, gD, features=f, dF=dF, camera_grads=True)
    assert _bits(Da, Db)
    for k in ("features",) + GRAD_NAMES + CAMERA:
        assert not torch.isnan(a[k]).any() and _bits(a[k], b[k]), k


# ------------------------------------------------------------------------------------------------ 7. NaN prefill
@pytest.mark.parametrize("name", ["A", "B"])
def test_nan_prefilled_outputs_are_fully_written(gpu_device, name, monkeypatch):
    """The map, the two totals and every gradient destination are written whole: torch.empty hands out NaN here, and
    the results have the bits of a fresh call, under bwd_prezero / bwd_live 0 and 1."""
    inp, dc, di = F.scene(name)
    n, W, H = AC.SCENES[name][:3]
    gD = DC.upstream(name)
    want, D = _run(inp, gpu_device, "z", dc, di, gD)
    real_empty = torch.empty

    def nan_empty(*a, **kw):
        t = real_empty(*a, **kw)
        return t.fill_(float("nan")) if t.is_floating_point() else t

    for prezero, live in ((1, 1), (0, 1), (1, 0), (0, 0)):
        with monkeypatch.context() as m:
            m.setattr(torch, "empty", nan_empty)
            from gaussian_splatting_lightning_amd import _native
            with _native.tuned(bwd_prezero=prezero, bwd_live=live):
                rs, res = _forward(inp, gpu_device, "z")
                st = res[-1]
                assert not torch.isnan(res[-2]).any() and not torch.isnan(st.distortion.totals).any()
                from gaussian_splatting_lightning_amd.rasterizer import backward_raw
                got = backward_raw(st, rs, _t(dc, gpu_device), _t(di, gpu_device), grad_out_distortion=_t(gD, gpu_device))
                torch.cuda.synchronize()
        assert _bits(res[-2], D)
        for k in GRAD_NAMES:  # (up to the sign of a zero: the zero fill's +0 or the per-Gaussian arithmetic's -0)
            assert not torch.isnan(got[k]).any() and torch.equal(got[k], want[k]), (k, prezero, live)


# ------------------------------------------------------------------------------------------------ 8. autograd
def test_autograd_surface(gpu_device):
    from gaussian_splatting_lightning_amd import GaussianRasterizer
    inp, dc, di = F.scene("A")
    dev = gpu_device
    f, dF = F.inputs("A", C_FEAT)
    gD = DC.upstream("A")
    n, W, H = AC.SCENES["A"][:3]

    def leaves():
        lv = {k: _t(inp[k], dev).requires_grad_(True) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
        lv["features"] = _t(f, dev).requires_grad_(True)
        lv["means2D"] = torch.zeros(n, 3, device=dev, requires_grad=True)
        return lv

    def call(rast, lv, **kw):
        return rast(means3D=lv["means3D"], means2D=lv["means2D"], opacities=lv["opacities"], shs=lv["shs"],
                    scales=lv["scales"], rotations=lv["rotations"], **kw)

    # the map is the last output, after alpha and the feature image; without distortion the call is what it was
    lv = leaves()
    out = call(GaussianRasterizer(settings_for(inp, dev), return_alpha=True, **_dist_kw("ndc")), lv,
               features=lv["features"])
    assert len(out) == 6 and out[4].shape == (C_FEAT, H, W) and out[5].shape == (1, H, W) and out[5].requires_grad
    assert len(call(GaussianRasterizer(settings_for(inp, dev), return_alpha=True), leaves())) == 4
    # a loss on the map alone
    lv = leaves()
    color, radii, invd, D = call(GaussianRasterizer(settings_for(inp, dev), **_dist_kw("z")), lv)
    (D * _t(gD, dev)).sum().backward()
    raw, _ = _run(inp, dev, "z", gD=gD)
    rec = {}
    for k in ("means3D", "opacities", "scales", "rotations", "means2D"):
        assert lv[k].grad is not None and float(lv[k].grad.abs().max()) > 0, k
        rec[k] = rel_l2(lv[k].grad.cpu().numpy(), raw[k].cpu().numpy().reshape(lv[k].grad.shape))
    # the joint loss, features included
    lv = leaves()
    color, radii, invd, image, D = call(GaussianRasterizer(settings_for(inp, dev), **_dist_kw("z")), lv,
                                        features=lv["features"])
    ((color * _t(dc, dev)).sum() + (invd * _t(di, dev)).sum() + (image * _t(dF, dev)).sum()
     + (D * _t(gD, dev)).sum()).backward()
    raw, _ = _run(inp, dev, "z", dc, di, gD, features=f, dF=dF)
    for k in ("features", "means3D", "shs", "opacities"):
        rec["joint_" + k] = rel_l2(lv[k].grad.cpu().numpy(), raw[k].cpu().numpy().reshape(lv[k].grad.shape))
    parity.record("distortion_autograd_A", "autograd_vs_backward_raw", dict(rec, bar=GRAD_TOL_ADHOC))
    print(rec)
    for k, v in rec.items():
        assert v <= GRAD_TOL_ADHOC, (k, v)


# ------------------------------------------------------------------------------------------------ 9. empty scenes
def test_empty_scenes(gpu_device):
    from gaussian_splatting_lightning_amd.rasterizer import backward_raw, forward_raw
    inp, dc, di = F.scene("A")
    dev = gpu_device
    n, W, H = AC.SCENES["A"][:3]
    gD = DC.upstream("A")
    rs = settings_for(inp, dev)
    e = lambda *s: torch.zeros(0, *s, device=dev)  # noqa: E731
    color, radii, invd, D, st = forward_raw(e(3), e(16, 3), None, e(1), e(3), e(4), None, rs, **_dist_kw("ndc"))
    g = backward_raw(st, rs, _t(dc, dev), _t(di, dev), grad_out_distortion=_t(gD, dev))
    torch.cuda.synchronize()
    assert D.shape == (1, H, W) and torch.all(D == 0) and torch.all(st.distortion.totals == 0)
    assert g["means3D"].shape == (0, 3)
    # every Gaussian behind the camera: nothing rendered, zeros and no launch fault
    ph = np.asarray([0.0, 0.0, -1.0, 1.0]) @ np.linalg.inv(inp["viewmatrix"].astype(np.float64))
    behind = dict(inp, means3D=(inp["means3D"] * f32(0.01) + (ph[:3] / ph[3]).astype(f32)).astype(f32))
    for which in DC.MAPS:
        g, D = _run(behind, dev, which, dc, di, gD, camera_grads=True)
        assert torch.all(g["radii"] == 0) and torch.all(D == 0)
        assert torch.all(g["means3D"] == 0) and torch.all(g["opacities"] == 0) and torch.all(g["viewmatrix"] == 0)


# ------------------------------------------------------------------------------------------------ 10. refusals
def test_refusals_on_the_device_path(gpu_device):
    from gaussian_splatting_lightning_amd import GaussianRasterizer
    from gaussian_splatting_lightning_amd.rasterizer import backward_chunked, backward_raw
    inp, dc, di = F.scene("A")
    dev = gpu_device
    n = AC.SCENES["A"][0]
    gD = DC.upstream("A")
    rs, res = _forward(inp, dev, "z")
    st = res[-1]
    with pytest.raises(NotImplementedError):
        backward_raw(st, rs, _t(dc, dev), _t(di, dev), grad_out_distortion=_t(gD, dev), absgrad=True)
    with pytest.raises(NotImplementedError):
        backward_chunked(st, rs, _t(dc, dev), _t(di, dev), [(0, n, {})])
    with pytest.raises(NotImplementedError):
        GaussianRasterizer(rs, absgrad=True, distortion="z")(
            means3D=_t(inp["means3D"], dev), means2D=None, opacities=_t(inp["opacities"], dev),
            shs=_t(inp["shs"], dev), scales=_t(inp["scales"], dev), rotations=_t(inp["rotations"], dev))
    with pytest.raises(RuntimeError, match="needs a state"):
        backward_raw(_forward(inp, dev)[1][-1], rs, _t(dc, dev), grad_out_distortion=_t(gD, dev))
    # the state still serves a plain backward afterwards
    g = backward_raw(st, rs, _t(dc, dev), _t(di, dev), grad_out_distortion=_t(gD, dev))
    torch.cuda.synchronize()
    assert float(g["means3D"].abs().max()) > 0
