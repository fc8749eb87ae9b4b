"""Mip-Splatting's 3D smoothing filter (csrc/gsr_mipfilter.hip, mipfilter.py), the parts that need no GPU: the three
exported symbols and their declarations, every argument refusal before any device work, the empty calls, the Python
validation errors, the camera table's layout, the identities of the float64 restatement the GPU tests are measured
against, the fp32 underflow that is the reason for the ratio form, and the conditions the scene generators assert."""
import ctypes
import os
import re

import pytest
import torch

from gaussian_splatting_lightning_amd import _native
from tests import mipfilter_cases as C

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gsrast.h")
GSR_OK, GSR_ERR_ARG = 0, 1
NAMES = ("gsr_mipfilter_rate", "gsr_activations_filter3d_forward", "gsr_activations_filter3d_backward")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_library_exports_the_entry_points():
    lib = _native.load()
    for name in NAMES:
        assert name in _native.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert re.search(r"\bint " + name + r"\(", _header()), name
        assert getattr(lib, name).restype is ctypes.c_int
    assert lib.gsr_abi_version() == _native.ABI_VERSION == 3  # new entry points, not a new ABI


def test_ctypes_signatures_match_the_header():
    lib = _native.load()
    kinds = {"ptr": ctypes.c_void_p, "int64_t": ctypes.c_int64, "int": ctypes.c_int, "float": ctypes.c_float}
    for name in NAMES:
        body = re.search(r"\bint " + name + r"\((.*?)\);", _header(), flags=re.S).group(1)
        want = []
        for prm in body.split(","):
            prm = " ".join(prm.split())
            want.append("ptr" if "*" in prm else prm.rsplit(" ", 1)[0].replace("const ", ""))
        got = getattr(lib, name).argtypes
        assert [kinds[w] for w in want] == list(got), name
    assert len(lib.gsr_mipfilter_rate.argtypes) == 9
    assert len(lib.gsr_activations_filter3d_forward.argtypes) == 9
    assert len(lib.gsr_activations_filter3d_backward.argtypes) == 12


def _refused(rc, lib, what):
    # on a host without a GPU a device call would give GSR_ERR_HIP (2): GSR_ERR_ARG shows the refusal came first
    assert rc == GSR_ERR_ARG, (what, rc)
    msg = lib.gsr_last_error()
    assert b"mipfilter" in msg or b"filter3d" in msg, what


def test_invalid_arguments_fail_before_any_device_work():
    lib = _native.load()
    P = 4096  # a made-up, 64-B aligned address
    # rate: (P, means3D, V, cameras, near, rate, zmin, seen, stream)
    ok = [5, P, 3, P, 0.2, P, P, P, None]
    for i in (1, 3, 5, 6, 7):
        a = list(ok)
        a[i] = None
        _refused(lib.gsr_mipfilter_rate(*a), lib, f"rate null {i}")
    for i, bad in ((0, -1), (2, 0), (2, -4), (4, float("nan")), (4, float("inf")), (4, -float("inf")), (3, P + 4)):
        a = list(ok)
        a[i] = bad
        _refused(lib.gsr_mipfilter_rate(*a), lib, f"rate arg {i} = {bad}")
    a = list(ok)
    a[0], a[2] = 0, 0  # no Gaussians does not excuse no cameras
    _refused(lib.gsr_mipfilter_rate(*a), lib, "rate P = 0, V = 0")
    # forward: (N, scaling, opacity, rotation, filter_3D, scales, opacities, rotations, stream)
    ok = [5] + [P] * 7 + [None]
    for i in range(1, 8):
        a = list(ok)
        a[i] = None
        _refused(lib.gsr_activations_filter3d_forward(*a), lib, f"forward null {i}")
    a = list(ok)
    a[0] = -1
    _refused(lib.gsr_activations_filter3d_forward(*a), lib, "forward N < 0")
    for i in (3, 7):
        a = list(ok)
        a[i] = P + 4
        _refused(lib.gsr_activations_filter3d_forward(*a), lib, f"forward misaligned {i}")
    # backward: (N, scaling, opacity, rotation, filter_3D, dL_dscales, dL_dopacities, dL_drotations, dL_dscaling,
    #            dL_dopacity, dL_drotation, stream)
    ok = [5] + [P] * 10 + [None]
    for i in range(1, 11):
        a = list(ok)
        a[i] = None
        _refused(lib.gsr_activations_filter3d_backward(*a), lib, f"backward null {i}")
    a = list(ok)
    a[0] = -1
    _refused(lib.gsr_activations_filter3d_backward(*a), lib, "backward N < 0")
    for i in (3, 7, 10):
        a = list(ok)
        a[i] = P + 8
        _refused(lib.gsr_activations_filter3d_backward(*a), lib, f"backward misaligned {i}")


def test_empty_calls_launch_nothing():
    """P = 0 / N = 0: GSR_OK without a device call (which would be GSR_ERR_HIP here, and a fault at these addresses)."""
    lib = _native.load()
    P = 4096
    assert lib.gsr_mipfilter_rate(0, P, 3, P, 0.2, P, P, P, None) == GSR_OK
    assert lib.gsr_activations_filter3d_forward(*([0] + [P] * 7 + [None])) == GSR_OK
    assert lib.gsr_activations_filter3d_backward(*([0] + [P] * 10 + [None])) == GSR_OK


def test_python_argument_validation():
    from gaussian_splatting_lightning_amd import mipfilter as M
    means, cams = C.scene("one_camera")
    for bad in (torch.zeros(5, 4), torch.zeros(5), torch.zeros(5, 3, dtype=torch.float64), [[0.0] * 3]):
        with pytest.raises(ValueError, match="means3D"):
            M.sampling_rate(bad, cams)
    with pytest.raises(ValueError, match="device tensor"):  # a CPU tensor: there is no CPU path
        M.sampling_rate(means, cams)
    with pytest.raises(ValueError, match="device tensor"):
        M.compute_3d_filter(means, C.as_settings(cams))
    empty = {k: v[:0] for k, v in cams.items()}
    for fn in (M.sampling_rate, M.compute_3d_filter):
        for none in ([], (), empty):
            with pytest.raises(ValueError, match="cameras is empty"):
                fn(means, none)
        with pytest.raises(ValueError, match="lacks"):
            fn(means, {k: v for k, v in cams.items() if k != "width"})
        with pytest.raises(ValueError, match=r"viewmatrix \(V,4,4\)"):
            fn(means, dict(cams, viewmatrix=cams["viewmatrix"][:, :3]))
        with pytest.raises(ValueError, match=r"viewmatrix \(V,4,4\)"):
            fn(means, dict(cams, tanfovy=torch.ones(2, dtype=torch.float64)))
        with pytest.raises(ValueError, match="near"):
            fn(means, cams, near=float("nan"))
        with pytest.raises(ValueError, match="margin"):
            fn(means, cams, margin=-0.1)
    for mode in ("shared", "", None):
        with pytest.raises(ValueError, match="mode must be"):
            M.compute_3d_filter(means, cams, mode=mode)
    with pytest.raises(ValueError, match="variance"):
        M.compute_3d_filter(means, cams, variance=-1.0)
    s, o, q, f = C.activation_inputs("ordinary", 8)
    shape = "expected scaling"
    for args, what in (((s[:, :2], o, q, f), shape), ((s, o[:7], q, f), shape), ((s, o, q[:, :3], f), shape),
                       ((s, o, q, f[:5]), shape), ((s, o, q, f.reshape(2, 2, 2)), shape),
                       ((s.double(), o, q, f), "fp32 device"), ((s, o, q, f), "fp32 device")):
        with pytest.raises(ValueError, match=what):
            M.activate_filtered(*args)
    with pytest.raises(ValueError, match="out must hold"):
        M.activate_filtered(s, o, q, f, out=(s, o, q[:4]))
    ups = C.upstream(8)
    for args, what in (((s, o, q, f[:5], *ups), shape), ((s, o, q, f, ups[0][:4], ups[1], ups[2]), "gradient shapes"),
                       ((s, o, q, f, ups[0], ups[1], ups[2][:, :3]), "gradient shapes"),
                       ((s, o, q, f, *ups), "fp32 device")):
        with pytest.raises(ValueError, match=what):
            M.activate_filtered_backward(*args)
    with pytest.raises(ValueError, match="fp32 device"):
        M.FilteredGaussianActivations.apply(s, o, q, f)


def test_model_refuses_a_missing_or_stale_filter():
    """The getters name compute_3d_filter when there is no filter_3D or one of another length; no device is needed to
    be told so."""
    from gaussian_splatting_lightning_amd.gaussian_model import GaussianModel
    g = GaussianModel(sh_degree=0, device="cpu")
    assert g.filter_3D is None and "filter_3D" not in g.state_dict()
    g._xyz = torch.nn.Parameter(torch.zeros(6, 3))
    for call in (g.get_scaling_with_3D_filter, g.get_opacity_with_3D_filter, lambda: g.get_activated(filter_3d=True),
                 lambda: g.save_ply("unused.ply", with_filter=True), lambda: g.save_fused_ply("unused.ply")):
        with pytest.raises(RuntimeError, match="no filter_3D.*compute_3d_filter"):
            call()
    g.filter_3D = torch.zeros(5, 1)
    assert "filter_3D" in g.state_dict()
    with pytest.raises(RuntimeError, match="filter_3D of 5 rows for 6 Gaussians.*compute_3d_filter"):
        g.get_activated(filter_3d=True)
    assert not os.path.exists("unused.ply")


def test_camera_table_layout():
    """Row k = [V[:,2] | V[:,0] | V[:,1] | fx, limx, limy, 0] in fp32, from either form of `cameras`."""
    from gaussian_splatting_lightning_amd.mipfilter import camera_table
    cams = C.ring_cameras(4, tans=((0.6, 0.4), (0.35, 0.5)), sizes=((640, 426), (1920, 1080)))
    table, fx = camera_table(cams, margin=0.15, device="cpu")
    assert table.shape == (4, 16) and table.dtype == torch.float32 and table.is_contiguous()
    vm = cams["viewmatrix"]
    assert torch.equal(table[:, 0:4], vm[:, :, 2]) and torch.equal(table[:, 4:8], vm[:, :, 0])
    assert torch.equal(table[:, 8:12], vm[:, :, 1]) and torch.equal(table[:, 15], torch.zeros(4))
    assert torch.equal(table[:, 12], fx) and torch.equal(fx, C.focal(cams).float())
    assert torch.equal(table[:, 13], (1.3 * cams["tanfovx"]).float())
    assert torch.equal(table[:, 14], (1.3 * cams["tanfovy"]).float())
    table2, fx2 = camera_table(C.as_settings(cams), margin=0.15, device="cpu")
    assert torch.equal(table, table2) and torch.equal(fx, fx2)
    # the row-vector convention of the definition: z = p . V[:3,2] + V[3,2]
    p = torch.tensor([[0.3, -0.2, 0.4]])
    _, _, z = C.view_space(p, cams)
    want = p.double() @ vm.double()[:, :3, 2].t() + vm.double()[:, 3, 2]
    assert torch.allclose(z, want, rtol=0, atol=1e-15)


def test_restatement_identities():
    for case in C.RANGES:
        s, o, q, f = C.activation_inputs(case, 257)
        sf, of, rot = C.activations(s, o, q, f)
        ps, po, prot = C.plain_activations(s, o, q)
        assert torch.equal(rot, prot)
        # the compensation keeps the Gaussian's integral: o' prod s' = o prod s
        assert C.max_rel(of * sf.prod(1, keepdim=True), po * ps.prod(1, keepdim=True)) <= 1e-14, case
        if case == "zero":  # f = 0: the plain activations (sqrt(s^2) is s to an ulp in float64)
            assert C.max_rel(sf, ps) <= 2.0 ** -52 and C.max_rel(of, po) <= 4 * 2.0 ** -52
        else:
            assert bool((sf > ps).all()) and bool((of < po).all())
        if case != "needle":  # well scaled: the published form is the ratio form (float64 carries both)
            assert C.max_rel(C.activations(s, o, q, f, form="published")[1], of) <= 1e-14, case
    # the gradients of the definition, against autograd on the restatement
    s, o, q, f = C.activation_inputs("ordinary", 64)
    ups = C.upstream(64)
    gs, go, _ = C.activation_grads(s, o, q, f, ups)
    s64, o64 = torch.exp(s.double()), torch.sigmoid(o.double())
    sf, of, _ = C.activations(s, o, q, f)
    c = (s64 / sf).prod(1, keepdim=True)
    want_s = ups[0].double() * s64 ** 2 / sf + ups[1].double() * of * f.double() ** 2 / sf ** 2
    want_o = ups[1].double() * c * o64 * (1 - o64)
    assert C.rel_l2(gs, want_s) <= 1e-14 and C.rel_l2(go, want_o) <= 1e-14


def test_filter_modes_and_unseen_fill():
    means, cams = C.scene("ring5")
    rate, zmin, seen = C.sampling_rate(means, cams)
    vis = seen > 0
    assert bool((rate[~vis] == 0).all()) and bool(torch.isinf(zmin[~vis]).all())
    a = C.filter_3d(means, cams, mode="per_camera")
    b = C.filter_3d(means, cams, mode="shared_focal")
    # equal focals: max fx / z over the visible cameras is fx / min z
    assert len(set(C.focal(cams).tolist())) == 1 and C.max_rel(a, b) <= 1e-14
    assert a.shape == (1000, 1) and bool((a[~vis] == a[vis].max()).all()) and bool((a > 0).all())
    assert C.max_rel(a[vis, 0], C.VARIANCE ** 0.5 / rate[vis]) <= 1e-15
    # different focals: the two modes differ, shared_focal the smaller or equal (it takes the largest focal)
    means, cams = C.scene("ring300")
    a, b = C.filter_3d(means, cams, mode="per_camera"), C.filter_3d(means, cams, mode="shared_focal")
    assert bool((b <= a * (1 + 1e-15)).all()) and float((a / b).max()) > 1.5
    # nothing seen at all: the identity
    means, cams = C.scene("unseen")
    assert int(C.sampling_rate(means, cams)[2].sum()) == 0
    for mode in ("per_camera", "shared_focal"):
        assert bool((C.filter_3d(means, cams, mode=mode) == 0).all())


def test_published_form_underflows_in_fp32_where_the_ratio_form_does_not():
    """Why the compensation is a product of ratios: at raw scaling -17 and f = 1e-3, prod s^2 = e^-102 = 5.0e-45 is
    below the smallest normal fp32 number by seven orders: flushed to zero it makes the published
    sqrt(prod s^2 / prod s'^2) exactly 0, kept as a denormal it is 4 units of 1.4e-45 and the result is off by per cents
    (either is an underflow; which one depends on the host's denormal mode).  At -18 the product is below half the
    smallest denormal and the result is 0 in either mode.  The ratio form stays within 5e-7 of float64 from -19 to -1."""
    q, b = torch.tensor([[1.0, 0.0, 0.0, 0.0]]), torch.zeros(1, 1)
    f = torch.full((1, 1), 1e-3)

    def err(raw, form):
        a = torch.full((1, 3), float(raw))
        got = C.activations(a, b, q, f, dtype=torch.float32, form=form)[1]
        return float(got), C.max_rel(got, C.activations(a, b, q, f)[1])

    value, e = err(-17.0, "published")
    assert value == 0.0 or e > 1e-2
    assert err(-18.0, "published")[0] == 0.0
    for raw in (-17.0, -18.0):
        value, e = err(raw, "ratio")
        assert value > 0.0 and e <= 5e-7
    for raw in range(-19, 0):
        assert err(raw, "ratio")[1] <= 5e-7, raw


def test_scene_generators_hold_their_conditions():
    """No pair within 1e-4 relative of a threshold, nothing dropped, every category populated where promised."""
    shapes = dict(ring5=(1000, 5), one_camera=(257, 1), single=(1, 1), ring300=(513, 300), unseen=(65, 3))
    for name, (P, V) in shapes.items():
        means, cams = C.scene(name)  # asserts the clearance itself
        assert means.shape == (P, 3) and means.dtype == torch.float32 and cams["viewmatrix"].shape == (V, 4, 4), name
        vis, z, clear = C.thresholds(means, cams)
        assert vis.shape == (P, V) and float(clear.min()) > C.CLEARANCE, name
    means, cams = C.scene("ring5")
    vis, z, _ = C.thresholds(means, cams)
    seen = vis.sum(1)
    assert int((seen == 0).sum()) >= 50 and int((seen == 5).sum()) >= 100 and int((z <= C.NEAR).sum()) >= 50
    means, cams = C.scene("ring300")
    assert len(set(C.focal(cams).tolist())) == 3 and len(set(cams["width"].tolist())) == 3
    # the derived bars are what fp32 needs and no more: the fp32 CPU restatement stays inside them
    for name in C.SCENES:
        means, cams = C.scene(name)
        r64, z64, s64 = C.sampling_rate(means, cams)
        r32, z32, s32 = C.sampling_rate(means, cams, dtype=torch.float32)
        rb, zb = C.rate_bars(means, cams)
        assert torch.equal(s32, s64), name
        vis = s64 > 0
        assert bool(((r32.double() - r64).abs() <= rb).all()) and bool(((z32.double() - z64)[vis].abs() <= zb[vis]).all())
    means, cams, seen = C.boundary_points()
    assert means.shape == (12, 3) and int(seen.sum()) == 6
