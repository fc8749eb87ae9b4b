"""Per-Gaussian contribution statistics (gsr_contributions, contributions_raw, GaussianRasterizer.contributions,
GaussianModel.accumulate_contributions / prune_by_contribution) on the GPU.

Truth: tests/contrib_cases.py -- the CPU oracle alone, one backward per three pixels whose colour gradient is the
compositing weight of every Gaussian at those pixels, read from tests/golden/contrib.npz.  The scenes are those of
tests/absgrad_cases.py: no threshold-flip candidate in any of them, asserted from the oracle with every truth, so the
bars are the project's clean bars without a flip term and no Gaussian or pixel is left out of a comparison:
count is exact, a single weight is the feature image of a one-hot feature (COLOR_TOL), and wsum is what dL_dfeatures
is (GRAD_CLEAN_TOL).  Achieved figures: profiles/parity_contrib.json.
"""
import math

import numpy as np
import pytest
import torch

from tests import absgrad_cases as AC
from tests import contrib_cases as CC
from tests import parity
from tests import test_alpha_background as TAB
from tests.helpers import rel_l2, scene_inputs, settings_for
from tests.test_gpu_parity import COLOR_TOL, GRAD_CLEAN_TOL

pytestmark = pytest.mark.gpu

f32 = np.float32
KINDS = CC.KINDS
# every forward-form knob set of tests/test_alpha_background.py::test_every_forward_form_writes_alpha_and_the_image, as
# tests/test_features.py takes them
FORWARD_FORMS = next(m for m in TAB.test_every_forward_form_writes_alpha_and_the_image.pytestmark
                     if m.name == "parametrize").args[1]


def _t(a, dev):
    return None if a is None else torch.as_tensor(np.asarray(a, f32), device=dev)


def _forward(inp, dev, colors=None, features=None):
    """forward_raw on the scene: SH colours unless `colors` (P,3) is given.  Returns (settings, result tuple)."""
    from gaussian_splatting_lightning_amd.rasterizer import forward_raw
    rs = settings_for(inp, dev)
    kw = {} if features is None else dict(features=features)
    res = forward_raw(_t(inp["means3D"], dev), None if colors is not None else _t(inp["shs"], dev), _t(colors, dev),
                      _t(inp["opacities"], dev), _t(inp["scales"], dev), _t(inp["rotations"], dev), None, rs, **kw)
    return rs, res


def _contrib(inp, dev, m=None, knobs=None, **kw):
    """Forward + contributions_raw under the knobs: (dict on the device, radii)."""
    from gaussian_splatting_lightning_amd import _native
    from gaussian_splatting_lightning_amd.rasterizer import contributions_raw
    with _native.tuned(**(knobs or {})):
        rs, res = _forward(inp, dev)
        got = contributions_raw(res[-1], rs, pixel_weights=_t(m, dev), **kw)
        torch.cuda.synchronize()
    return got, res[1]


def _bits(a, b):
    if a.dtype == torch.int64:
        return a.shape == b.shape and torch.equal(a, b)
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _same(a, b):
    return all(_bits(a[k], b[k]) for k in KINDS)


def _check_parity(case, got, radii, truth):
    """The three outputs against a truth dict(count, wsum, wmax): records the achieved figures, then asserts."""
    n = len(truth["count"])
    assert got["count"].dtype == torch.int64 and got["wsum"].dtype == got["wmax"].dtype == torch.float32
    assert all(got[k].shape == (n,) for k in KINDS)
    c, s, mx = (got[k].cpu().numpy() for k in KINDS)
    rec = dict(count_mismatches=int((c != truth["count"]).sum()), wmax_maxabs=float(np.abs(mx - truth["wmax"]).max()),
               wmax_bar=COLOR_TOL, wsum_rel_l2=rel_l2(s, truth["wsum"]), wsum_bar=GRAD_CLEAN_TOL, gaussians=n,
               taken=int((truth["count"] > 0).sum()), pairs=int(truth["count"].sum()))
    parity.record(case, "contributions_vs_oracle", rec)
    print(case, rec)
    assert rec["count_mismatches"] == 0, rec  # element for element
    assert rec["wmax_maxabs"] <= COLOR_TOL, rec  # every Gaussian
    assert rec["wsum_rel_l2"] <= GRAD_CLEAN_TOL, rec
    none = (radii.cpu().numpy() == 0) | (truth["count"] == 0)
    for a in (c, s, mx):  # exact zeros (no -0 either: the bits)
        assert not a[none].view(np.int32 if a.dtype == f32 else np.int64).any()


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("name", CC.SCENES)
def test_parity(gpu_device, name, weighted):
    assert CC.flip_candidates(name) == 0
    m = CC.weights(name) if weighted else None
    got, radii = _contrib(CC.scene(name), gpu_device, m)
    _check_parity(f"contrib_{name}_{'weighted' if weighted else 'plain'}", got, radii, CC.fixture_truth(name, weighted))


# ------------------------------------------------------------------------------------------------ 2. the other route
def test_against_the_feature_gradient_route(gpu_device):
    """A scene too large for the per-pixel truth: wsum against the library's only other route to it, the gradient of a
    constant feature channel under the upstream gradient m (m >= 0: a zero weight adds nothing on either route)."""
    from gaussian_splatting_lightning_amd.rasterizer import backward_raw, contributions_raw
    dev = gpu_device
    n, W, H = 2000, 128, 128
    inp = scene_inputs(n, W, H, sh_degree=3, seed=21)
    rng = np.random.default_rng(22)
    m = rng.random((H, W), dtype=f32)
    m[rng.random((H, W), dtype=f32) < f32(0.25)] = f32(0.0)
    rs, res = _forward(inp, dev, features=torch.ones(n, 1, device=dev))
    st = res[-1]
    by_m = backward_raw(st, rs, None, grad_out_features=_t(m[None], dev))["features"][:, 0]
    by_1 = backward_raw(st, rs, None, grad_out_features=torch.ones(1, H, W, device=dev))["features"][:, 0]
    weighted = contributions_raw(st, rs, pixel_weights=_t(m, dev))
    plain = contributions_raw(st, rs)
    torch.cuda.synchronize()
    rec = dict(wsum_weighted_rel_l2=rel_l2(weighted["wsum"].cpu().numpy(), by_m.cpu().numpy()),
               wsum_plain_rel_l2=rel_l2(plain["wsum"].cpu().numpy(), by_1.cpu().numpy()), bar=2 * GRAD_CLEAN_TOL,
               taken=int((plain["count"] > 0).sum()), instances=int(st.num_rendered), num_big=int(st.num_big))
    parity.record("contrib_vs_feature_gradient_2000_128", "wsum_vs_dL_dfeatures", rec)
    print(rec)
    assert rec["wsum_weighted_rel_l2"] <= 2 * GRAD_CLEAN_TOL and rec["wsum_plain_rel_l2"] <= 2 * GRAD_CLEAN_TOL, rec
    assert torch.equal(plain["count"] > 0, by_1 != 0) and 0 < rec["taken"] < n
    assert torch.all(plain["wmax"] <= plain["wsum"]) and torch.all(plain["wmax"] <= 0.99)
    assert torch.all(weighted["count"] <= plain["count"]) and torch.all(weighted["wmax"] <= plain["wmax"])
    assert torch.all((plain["count"] > 0) == (plain["wmax"] > 0))


# ------------------------------------------------------------------------------------------------ 3. forms, guard
@pytest.mark.parametrize("knobs", FORWARD_FORMS, ids=lambda k: "-".join(f"{n}{v}" for n, v in k.items()))
def test_every_forward_form_gives_the_same_bits(gpu_device, knobs):
    for name in ("A", "B"):
        inp, m = CC.scene(name), CC.weights(name)
        want, _ = _contrib(inp, gpu_device, m)
        got, _ = _contrib(inp, gpu_device, m, knobs=knobs)
        assert _same(got, want), name  # the walk reads only recorded state


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_parity_under_the_guard(gpu_device, weighted):
    """The forward and the call both under "guard": the guarded decisions, replayed."""
    assert CC.flip_candidates("A") == 0
    got, radii = _contrib(CC.scene("A"), gpu_device, CC.weights("A") if weighted else None, knobs=dict(guard=1))
    _check_parity(f"contrib_A_guard_{'weighted' if weighted else 'plain'}", got, radii, CC.fixture_truth("A", weighted))


# ------------------------------------------------------------------------------------------------ 4. repeat, scratch
@pytest.mark.parametrize("name", ["A2", "B"])
def test_calls_repeat_and_leave_no_trace_in_scratch_or_outputs(gpu_device, name):
    from gaussian_splatting_lightning_amd import _native
    from gaussian_splatting_lightning_amd.rasterizer import contributions_raw
    dev = gpu_device
    n = AC.SCENES[name][0]
    m = _t(CC.weights(name), dev)
    rs, res = _forward(CC.scene(name), dev)
    st = res[-1]
    first = contributions_raw(st, rs, pixel_weights=m)
    again = contributions_raw(st, rs, pixel_weights=m)
    assert _same(first, again) and not torch.isnan(first["wsum"]).any() and int(first["count"].sum()) > 0
    # the caching allocator hands the block of a freed tensor of the scratch's size to the next call: all-ones bytes
    # (NaN as floats, 2^32 - 1 as counts) where the rows of instances no wave loaded stay unwritten
    nbytes = _native.load().gsr_contrib_scratch_bytes(st.num_rendered, st.num_big)
    junk = torch.empty(nbytes, dtype=torch.uint8, device=dev).fill_(255)
    del junk
    assert _same(contributions_raw(st, rs, pixel_weights=m), first)
    # NaN-prefilled outputs come back fully written
    out = dict(count=torch.full((n,), -7, dtype=torch.int64, device=dev), wsum=torch.full((n,), float("nan"), device=dev),
               wmax=torch.full((n,), float("nan"), device=dev))
    got = contributions_raw(st, rs, pixel_weights=m, out=out)
    assert all(got[k].data_ptr() == out[k].data_ptr() for k in KINDS) and _same(got, first)
    # each output alone
    for k in KINDS:
        alone = contributions_raw(st, rs, pixel_weights=m, out={k: torch.empty_like(first[k])})
        assert _bits(alone[k], first[k]) and all(alone[o] is None for o in KINDS if o != k), k


# ------------------------------------------------------------------------------------------------ 5. accumulate
def test_accumulate_over_two_views(gpu_device):
    from gaussian_splatting_lightning_amd.rasterizer import contributions_raw
    dev = gpu_device
    n = AC.SCENES["A"][0]
    per_view = []
    buf = dict(count=torch.zeros(n, dtype=torch.int64, device=dev), wsum=torch.zeros(n, device=dev),
               wmax=torch.zeros(n, device=dev))
    for name in ("A", "A2"):  # the same P
        rs, res = _forward(CC.scene(name), dev)
        per_view.append(contributions_raw(res[-1], rs, pixel_weights=_t(CC.weights(name), dev)))
        got = contributions_raw(res[-1], rs, pixel_weights=_t(CC.weights(name), dev), out=buf, accumulate=True)
        assert all(got[k] is buf[k] for k in KINDS)
    a, b = per_view
    assert torch.equal(buf["count"], a["count"] + b["count"])
    assert _bits(buf["wsum"], a["wsum"] + b["wsum"])  # one fp32 add
    assert _bits(buf["wmax"], torch.maximum(a["wmax"], b["wmax"]))
    assert not _bits(a["wsum"], b["wsum"]) and int(b["count"].sum()) > int(a["count"].sum())


# ------------------------------------------------------------------------------------------------ 6. read only
@pytest.mark.parametrize("name", ["A", "B"])
def test_the_state_is_only_read(gpu_device, name):
    from gaussian_splatting_lightning_amd.rasterizer import backward_raw, contributions_raw
    dev = gpu_device
    inp, dc, di = AC.scene(name, None)
    inp = CC.scene(name)
    rs, res = _forward(inp, dev)
    without = backward_raw(res[-1], rs, _t(dc, dev), _t(di, dev), absgrad=True)
    rs, res2 = _forward(inp, dev)
    contributions_raw(res2[-1], rs, pixel_weights=_t(CC.weights(name), dev))
    contributions_raw(res2[-1], rs)
    after = backward_raw(res2[-1], rs, _t(dc, dev), _t(di, dev), absgrad=True)
    torch.cuda.synchronize()
    for k in ("means3D", "means2D", "opacities", "scales", "rotations", "shs", "means2D_abs"):
        assert not torch.isnan(after[k]).any() and _bits(after[k], without[k]), k
    _, res3 = _forward(inp, dev)
    for i in (0, 2):  # colour, inverse depth
        assert _bits(res3[i], res[i]) and _bits(res2[i], res[i])
    assert torch.equal(res3[1], res[1])


# ------------------------------------------------------------------------------------------------ 7. empty cases
def test_empty_cases(gpu_device):
    from gaussian_splatting_lightning_amd.rasterizer import contributions_raw, forward_raw
    dev = gpu_device
    inp = CC.scene("A")
    n = AC.SCENES["A"][0]
    rs = settings_for(inp, dev)
    e = lambda *s: torch.zeros(0, *s, device=dev)  # noqa: E731
    st = forward_raw(e(3), e(16, 3), None, e(1), e(3), e(4), None, rs)[-1]
    got = contributions_raw(st, rs)
    assert got["count"].shape == (0,) and got["count"].dtype == torch.int64 and got["wsum"].shape == (0,)
    # every Gaussian behind the camera: nothing rendered
    ph = np.asarray([0.0, 0.0, -1.0, 1.0]) @ np.linalg.inv(inp["viewmatrix"].astype(np.float64))
    behind = dict(inp, means3D=(inp["means3D"] * f32(0.01) + (ph[:3] / ph[3]).astype(f32)).astype(f32))
    rs, res = _forward(behind, dev)
    assert res[-1].num_rendered == 0 and torch.all(res[1] == 0)
    out = dict(count=torch.full((n,), -7, dtype=torch.int64, device=dev), wsum=torch.full((n,), float("nan"), device=dev),
               wmax=torch.full((n,), float("nan"), device=dev))
    got = contributions_raw(res[-1], rs, out=out)
    torch.cuda.synchronize()
    for k in KINDS:
        assert not got[k].view(torch.int64 if k == "count" else torch.int32).any(), k  # zeros, bit for bit
    # under accumulate the buffers are left as they are
    out = dict(count=torch.full((n,), 5, dtype=torch.int64, device=dev), wsum=torch.full((n,), 1.5, device=dev),
               wmax=torch.full((n,), 0.25, device=dev))
    contributions_raw(res[-1], rs, out=out, accumulate=True)
    torch.cuda.synchronize()
    assert torch.all(out["count"] == 5) and torch.all(out["wsum"] == 1.5) and torch.all(out["wmax"] == 0.25)


# ------------------------------------------------------------------------------------------------ 8. surface
def test_module_and_functional_surface(gpu_device):
    from gaussian_splatting_lightning_amd import GaussianRasterizer, rasterize_contributions
    dev = gpu_device
    inp = CC.scene("A")
    n = AC.SCENES["A"][0]
    m = _t(CC.weights("A"), dev)
    want, radii = _contrib(inp, dev, CC.weights("A"))
    rast = GaussianRasterizer(settings_for(inp, dev))
    geo = dict(means3D=_t(inp["means3D"], dev).requires_grad_(True), opacities=_t(inp["opacities"], dev),
               scales=_t(inp["scales"], dev), rotations=_t(inp["rotations"], dev))
    colours = (dict(shs=_t(inp["shs"], dev)), dict(colors_precomp=torch.rand(n, 3, device=dev)), dict())
    for kw in colours:
        got, r = rast.contributions(pixel_weights=m[None], **geo, **kw)
        assert _same(got, want) and torch.equal(r, radii), list(kw)
        assert not any(got[k].requires_grad for k in KINDS)
    got, r = rasterize_contributions(geo["means3D"], geo["opacities"], rast.raster_settings, scales=geo["scales"],
                                     rotations=geo["rotations"], pixel_weights=m)
    assert _same(got, want) and torch.equal(r, radii)
    plain, _ = rast.contributions(**geo)
    assert _same(plain, _contrib(inp, dev)[0]) and not _bits(plain["wsum"], want["wsum"])


# ------------------------------------------------------------------------------------------------ 9. model
def _model(dev):
    """Scene A's Gaussians in a GaussianModel with GaussianAdam state and non-trivial densification statistics."""
    from gaussian_splatting_lightning_amd.gaussian_model import GaussianModel
    from gaussian_splatting_lightning_amd.optim import GaussianAdam
    inp = CC.scene("A")
    n = AC.SCENES["A"][0]
    model = GaussianModel(sh_degree=3, spatial_scale=1.0, device=dev)
    op = np.clip(inp["opacities"].astype(np.float64), 1e-6, 1 - 1e-6)
    model._set_params(dict(xyz=_t(inp["means3D"], dev), features_dc=_t(inp["shs"][:, :1], dev).contiguous(),
                           features_rest=_t(inp["shs"][:, 1:], dev).contiguous(),
                           opacity=_t(np.log(op / (1 - op)), dev).reshape(n, 1), scaling=_t(np.log(inp["scales"]), dev),
                           rotation=_t(inp["rotations"], dev), active_sh_degree=3))
    gen = torch.Generator(device=dev).manual_seed(5)
    model.xyz_grad_accum = torch.rand(n, device=dev, generator=gen)
    model.xyz_grad_count = torch.randint(0, 6, (n,), device=dev, generator=gen).float()
    model.max_radii2D = torch.rand(n, device=dev, generator=gen) * 40
    lrs = dict(xyz=1.6e-4, features_dc=2.5e-3, features_rest=1.25e-4, opacity=0.025, scaling=5e-3, rotation=1e-3)
    opt = GaussianAdam([{"params": [getattr(model, f"_{k}")], "lr": lrs[k], "name": k} for k in model.PARAMETER_NAMES],
                       lr=0.0, eps=1e-15)
    for k in model.PARAMETER_NAMES:
        prm = getattr(model, f"_{k}")
        opt.state[prm] = dict(step=torch.tensor(5.0), exp_avg=torch.randn(prm.shape, device=dev, generator=gen),
                              exp_avg_sq=torch.rand(prm.shape, device=dev, generator=gen))
    return model, opt


def _snapshot(model, opt):
    snap = {}
    for k in model.PARAMETER_NAMES:
        prm = getattr(model, f"_{k}")
        snap[k] = (prm.detach().clone(), opt.state[prm]["exp_avg"].clone(), opt.state[prm]["exp_avg_sq"].clone())
    for k in ("xyz_grad_accum", "xyz_grad_count", "max_radii2D"):
        snap[k] = getattr(model, k).clone()
    return snap


def _check_pruned(model, opt, snap, keep, idx):
    assert torch.equal(idx, keep.nonzero().squeeze(-1)) and idx.dtype == torch.int64
    for k in model.PARAMETER_NAMES:
        prm = getattr(model, f"_{k}")
        assert isinstance(prm, torch.nn.Parameter) and _bits(prm.detach(), snap[k][0][keep]), k
        grp = [g for g in opt.param_groups if g["name"] == k][0]
        assert grp["params"][0] is prm and float(opt.state[prm]["step"]) == 5.0
        assert _bits(opt.state[prm]["exp_avg"], snap[k][1][keep]) and _bits(opt.state[prm]["exp_avg_sq"], snap[k][2][keep])
    assert len(opt.state) == len(model.PARAMETER_NAMES)
    for k in ("xyz_grad_accum", "xyz_grad_count", "max_radii2D"):
        assert _bits(getattr(model, k), snap[k][keep]), k
    assert model.contrib_count is None and model.contrib_wsum is None and model.contrib_wmax is None  # dropped


def test_model_accumulates_and_prunes(gpu_device):
    from gaussian_splatting_lightning_amd import GaussianRasterizer
    from gaussian_splatting_lightning_amd.rasterizer import contributions_raw
    dev = gpu_device
    inp = CC.scene("A")
    n, W, H, seed = AC.SCENES["A"][:4]
    other = scene_inputs(n, W, H, sh_degree=3, seed=seed, view_index=1, num_views=4)
    views = [inp, dict(inp, **{k: other[k] for k in ("viewmatrix", "projmatrix", "campos")})]

    def render_args(model):
        return dict(means3D=model.get_xyz(), opacities=model.get_opacity(), shs=model.get_features(),
                    scales=model.get_scaling(), rotations=model.get_rotation())

    model, opt = _model(dev)
    assert model.contrib_count is None
    separate = []
    for i, view in enumerate(views):
        rast = GaussianRasterizer(settings_for(view, dev))
        separate.append(rast.contributions(**render_args(model))[0])
        if i == 0:
            model.accumulate_contributions(rasterizer=rast, **render_args(model))  # straight into the buffers
        else:
            model.accumulate_contributions(separate[-1])  # a stats dict
    a, b = separate
    assert int(b["count"].sum()) > 0 and not torch.equal(a["count"], b["count"])
    assert model.contrib_count.dtype == torch.int64 and torch.equal(model.contrib_count, a["count"] + b["count"])
    assert _bits(model.contrib_wsum, a["wsum"] + b["wsum"]) and _bits(model.contrib_wmax, torch.maximum(a["wmax"], b["wmax"]))
    # threshold
    t = float(model.contrib_wmax[model.contrib_wmax > 0].median())
    keep = model.contrib_wmax > t
    assert 0 < int(keep.sum()) < n and bool((~keep & (model.contrib_wmax > 0)).any())
    snap = _snapshot(model, opt)
    idx = model.prune_by_contribution("wmax", threshold=t, optimizer=opt)
    torch.cuda.synchronize()
    _check_pruned(model, opt, snap, keep, idx)
    # keep_ratio on the pruned model: fresh buffers of the new size, the top half by wsum
    n1 = int(keep.sum())
    model.accumulate_contributions(rasterizer=GaussianRasterizer(settings_for(inp, dev)), **render_args(model))
    assert model.contrib_wsum.shape == (n1,)
    order = torch.sort(model.contrib_wsum, descending=True, stable=True).indices
    keep2 = torch.zeros(n1, dtype=torch.bool, device=dev)
    keep2[order[:math.ceil(0.5 * n1)]] = True
    snap = _snapshot(model, opt)
    idx = model.prune_by_contribution("wsum", keep_ratio=0.5, optimizer=opt)
    _check_pruned(model, opt, snap, keep2, idx)
    assert model._xyz.shape[0] == math.ceil(0.5 * n1)
    # ties go to the lower index: a score of seven levels, 3/7 of the rows kept
    n2 = model._xyz.shape[0]
    score = (torch.arange(n2, device=dev) % 7).float()
    k2 = math.ceil(0.4 * n2)
    want = np.zeros(n2, bool)
    want[np.argsort(-score.cpu().numpy(), kind="stable")[:k2]] = True
    level = score.cpu().numpy()[want].min()
    tied = np.flatnonzero(score.cpu().numpy() == level)
    assert 0 < want[tied].sum() < len(tied) and not want[tied][np.argmin(want[tied]):].any()  # a cut inside a tie
    snap = _snapshot(model, opt)
    idx = model.prune_by_contribution(score, keep_ratio=0.4, optimizer=opt)
    _check_pruned(model, opt, snap, torch.as_tensor(want, device=dev), idx)
    model.reset_contributions()
    assert model.contrib_wmax is None
    # training goes on: one optimizer step on the pruned model
    for k in model.PARAMETER_NAMES:
        getattr(model, f"_{k}").grad = torch.ones_like(getattr(model, f"_{k}"))
    opt.step()
    torch.cuda.synchronize()
    assert torch.isfinite(model._xyz).all()


def test_densify_and_prune_gives_what_it_gave(gpu_device):
    """The rebind tail is shared with prune_points now: tests/test_densify.py's fixture against the numpy oracle, with
    the optimizer state."""
    from tests import test_densify as TD
    counts = TD._gpu_vs_oracle(5000, TD.THRESH[0], seed=11, with_optimizer=True)
    assert counts[1] > 0 and counts[2] > 0 and counts[0] < 5000
