"""Normal consistency (csrc/gsr_normals.hip, normals.py), the parts that need no GPU: the five exported symbols and
their declarations, every argument refusal before any device work, the empty calls, the Python-side refusals, and the
identities of the float64 restatement the GPU tests are measured against (a plane's depth image gives the plane's normal
and E = 1 - A^2), so the yardstick itself is checked."""
import ctypes
import os
import re

import pytest
import torch

from gaussian_splatting_lightning_amd import _native
from tests import normal_cases as C

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gsrast.h")
GSR_OK, GSR_ERR_ARG = 0, 1
ARGC = {"gsr_geomfeat_forward": 7, "gsr_geomfeat_backward": 9, "gsr_normal_consistency_forward": 10,
        "gsr_depth_to_normal": 8, "gsr_normal_consistency_backward": 12}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_library_exports_the_entry_points():
    lib = _native.load()
    for name in ARGC:
        assert name in _native.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert re.search(r"\bint " + name + r"\(", _header()), name
        assert getattr(lib, name).restype is ctypes.c_int
    assert lib.gsr_abi_version() == _native.ABI_VERSION == 3  # new entry points, not a new ABI


def test_ctypes_signatures_match_the_header():
    lib = _native.load()
    kinds = {"ptr": ctypes.c_void_p, "int64_t": ctypes.c_int64, "int": ctypes.c_int, "float": ctypes.c_float}
    for name, argc in ARGC.items():
        body = re.search(r"\bint " + name + r"\((.*?)\);", _header(), flags=re.S).group(1)
        want = []
        for prm in body.split(","):
            prm = " ".join(prm.split())
            want.append("ptr" if "*" in prm else prm.rsplit(" ", 1)[0].replace("const ", ""))
        got = getattr(lib, name).argtypes
        assert [kinds[w] for w in want] == list(got), name
        assert len(got) == argc, name


def _refused(rc, lib, what):
    # on a host without a GPU a device call would give GSR_ERR_HIP (2): GSR_ERR_ARG shows the refusal came first
    assert rc == GSR_ERR_ARG, (what, rc)
    msg = lib.gsr_last_error()
    assert b"geomfeat" in msg or b"normal consistency" in msg, what


BAD_TAN = (0.0, -0.5, float("nan"), float("inf"), -float("inf"))


def test_invalid_arguments_fail_before_any_device_work():
    lib = _native.load()
    P = 4096  # a made-up, aligned address
    # (P, means3D, scales, rotations, viewmatrix, out, stream)
    ok = [5] + [P] * 5 + [None]
    for i in range(1, 6):
        a = list(ok)
        a[i] = None
        _refused(lib.gsr_geomfeat_forward(*a), lib, f"geomfeat forward null {i}")
    _refused(lib.gsr_geomfeat_forward(*([-1] + ok[1:])), lib, "geomfeat forward P < 0")
    for i in (3, 5):
        a = list(ok)
        a[i] = P + 4
        _refused(lib.gsr_geomfeat_forward(*a), lib, f"geomfeat forward misaligned {i}")
    # (P, means3D, scales, rotations, viewmatrix, dL_dout, dL_dmeans3D, dL_drotations, stream)
    ok = [5] + [P] * 7 + [None]
    for i in range(1, 8):
        a = list(ok)
        a[i] = None
        _refused(lib.gsr_geomfeat_backward(*a), lib, f"geomfeat backward null {i}")
    _refused(lib.gsr_geomfeat_backward(*([-1] + ok[1:])), lib, "geomfeat backward P < 0")
    for i in (3, 5, 7):
        a = list(ok)
        a[i] = P + 8
        _refused(lib.gsr_geomfeat_backward(*a), lib, f"geomfeat backward misaligned {i}")
    # (H, W, tanfovx, tanfovy, then the arrays, stream); n_d of the forward (index 8) may be NULL
    for fn, n, optional in ((lib.gsr_normal_consistency_forward, 5, (8,)), (lib.gsr_depth_to_normal, 3, ()),
                            (lib.gsr_normal_consistency_backward, 7, ())):
        ok = [6, 9, 0.6, 0.45] + [P] * n + [None]
        for i in range(4, 4 + n):
            if i in optional:
                continue
            a = list(ok)
            a[i] = None
            _refused(fn(*a), lib, f"{fn.__name__} null {i}")
        for i in (0, 1):
            for bad in (0, -3):
                a = list(ok)
                a[i] = bad
                _refused(fn(*a), lib, f"{fn.__name__} arg {i} = {bad}")
        for i in (2, 3):
            for bad in BAD_TAN:
                a = list(ok)
                a[i] = bad
                _refused(fn(*a), lib, f"{fn.__name__} arg {i} = {bad}")
        a = list(ok)
        a[0], a[1] = 65536, 65536  # H * W above 2^31 - 1
        _refused(fn(*a), lib, f"{fn.__name__} too large")


def test_empty_calls_launch_nothing():
    """P = 0: GSR_OK without a device call (which would be GSR_ERR_HIP here, and a fault at these addresses)."""
    lib = _native.load()
    P = 4096
    assert lib.gsr_geomfeat_forward(*([0] + [P] * 5 + [None])) == GSR_OK
    assert lib.gsr_geomfeat_backward(*([0] + [P] * 7 + [None])) == GSR_OK


def _settings(H, W, tanfovx=0.6, tanfovy=0.45, viewmatrix=None):
    from gaussian_splatting_lightning_amd import GaussianRasterizationSettings
    vm = torch.eye(4) if viewmatrix is None else viewmatrix
    return GaussianRasterizationSettings(H, W, tanfovx, tanfovy, torch.zeros(3), 1.0, vm, torch.eye(4), 0,
                                         torch.zeros(3), False, False, False)


def test_python_argument_validation():
    """Refusals are ValueError before the device is asked for anything: this host has none."""
    from gaussian_splatting_lightning_amd import normals as M
    means, scales, rots, vm, _ = C.make_geometry(C.GEOMETRY_CASES[1])
    for bad, what in (((means[:, :2], scales, rots, vm), "means3D"), ((means, scales[:, :2], rots, vm), "scales"),
                      ((means, scales, rots[:, :3], vm), "rotations"), ((means, scales[:5], rots, vm), "same number"),
                      ((means, scales, rots, vm[:3]), "viewmatrix"), ((means, scales, rots, None), "viewmatrix"),
                      ((means.double(), scales, rots, vm), "fp32 device"),
                      ((means, scales, rots, vm), "fp32 device")):  # CPU tensors: there is no CPU path
        with pytest.raises(ValueError, match=what):
            M.geometry_features(*bad)
    with pytest.raises(ValueError, match="fp32 device"):
        M.geometry_features(means, scales, rots, _settings(4, 4, viewmatrix=vm))
    with pytest.raises(NotImplementedError, match="camera gradient"):
        M.geometry_features(means, scales, rots, vm.clone().requires_grad_(True))
    with pytest.raises(NotImplementedError, match="camera gradient"):
        M.geometry_features(means, scales, rots, _settings(4, 4, viewmatrix=vm.clone().requires_grad_(True)))
    D, A, N, _ = C.make(C.BY_NAME["5x7"])
    s = _settings(5, 7)
    for args, what in (((D, A, N, _settings(7, 5)), r"depth \(1,7,5\)"), ((D, A[:, :4], N, s), "alpha"),
                       ((D, A, N[:2], s), "normals"), ((D[0], A, N, s), "depth"),
                       ((D, A, N, _settings(5, 7, tanfovx=0.0)), "tanfovx"),
                       ((D, A, N, _settings(5, 7, tanfovy=float("nan"))), "tanfovx"),
                       ((D.double(), A, N, s), "fp32 device"), ((D, A, N, s), "fp32 device")):
        with pytest.raises(ValueError, match=what):
            M.normal_consistency(*args)
    for args, what in (((D, A, _settings(7, 5)), "depth"), ((D, A[:, :4], s), "alpha"), ((D, A, s), "fp32 device")):
        with pytest.raises(ValueError, match=what):
            M.depth_to_normal(*args)
    from gaussian_splatting_lightning_amd import GaussianRasterizer
    for r in (GaussianRasterizer(s), GaussianRasterizer(s, return_alpha=True, distortion="z")):
        with pytest.raises(ValueError, match="return_alpha=True"):
            M.render_normal_consistency(r, means, None, means[:, :1], colors_precomp=means, scales=scales,
                                        rotations=rots)
    with pytest.raises(ValueError, match="scales and rotations"):
        M.render_normal_consistency(GaussianRasterizer(s, return_alpha=True), means, None, means[:, :1],
                                    colors_precomp=means)


def test_model_has_the_getter():
    from gaussian_splatting_lightning_amd.gaussian_model import GaussianModel
    assert callable(GaussianModel.get_geometry_features)


def test_plane_identities_of_the_restatement():
    """float64: the depth image of the plane n . p = c gives n_d = n at every interior pixel, and with N = A n the map
    is E = 1 - A^2 there; E = 1 and n_d = 0 on the border."""
    case = C.BY_NAME["37x53-plane"]
    A = C.make(case)[1].double()
    n = torch.tensor(case.plane[:3], dtype=torch.float64).view(3, 1, 1)
    D = A * C.plane_depth(case)
    n_d = C.depth_normals(D, A, case.tanfovx, case.tanfovy)
    assert float((n_d[:, 1:-1, 1:-1] - n).abs().max()) <= 1e-13
    E = C.consistency(D, A, A * n, case.tanfovx, case.tanfovy)
    assert float((E - (1 - A * A))[:, 1:-1, 1:-1].abs().max()) <= 1e-14
    border = torch.ones(case.H, case.W, dtype=torch.bool)
    border[1:-1, 1:-1] = False
    assert bool((E[0][border] == 1).all()) and bool((n_d[:, border] == 0).all())
    # a fronto-parallel surface faces the camera the way the Gaussian normals do
    flat = C.depth_normals(2 * A, A, case.tanfovx, case.tanfovy)[:, 1:-1, 1:-1]
    assert float((flat - torch.tensor([0.0, 0.0, -1.0], dtype=torch.float64).view(3, 1, 1)).abs().max()) <= 1e-13


def test_restatement_edges():
    """No interior (H < 3 or W < 3): E == 1 and zero gradients.  A hole of alpha == 0: E == 1 and zero gradients at
    the pixels whose four neighbours are in it."""
    for name in ("2x7", "5x1"):
        E, dD, dA, dN = C.reference(C.BY_NAME[name])
        assert bool((E == 1).all()) and not dD.any() and not dA.any() and not dN.any()
    case = C.BY_NAME["37x53-hole"]
    y0, y1, x0, x1 = case.hole
    E, dD, dA, dN = C.reference(case)
    inner = (slice(None), slice(y0 + 1, y1 - 1), slice(x0 + 1, x1 - 1))
    assert bool((E[inner] == 1).all()) and not dD[inner].any() and not dA[inner].any() and not dN[inner].any()
    assert all(bool(torch.isfinite(t).all()) for t in (E, dD, dA, dN))


def test_geometry_restatement_and_cases():
    """The restated normal is a unit vector that faces the camera; about half of the rows need the flip; scales get no
    gradient; the conditions make() asserts hold for every case."""
    for case in C.GEOMETRY_CASES:
        means, scales, rots, vm, dg = (t.double() for t in C.make_geometry(case))
        g, dmeans, drots, dscales = C.run_geometry(means, scales, rots, vm, dg)
        p_view = means @ vm[:3, :3] + vm[3, :3]
        assert bool(((g[:, :3] * p_view).sum(1) < 0).all())
        assert torch.allclose(g[:, 3], p_view[:, 2])
        assert dscales is None or not dscales.any()
        assert torch.allclose(dmeans, dg[:, 3:4] * vm[:3, 2][None, :])
        # the gradient is tangent to the quaternion: scaling q changes nothing
        assert float((drots * rots).sum(1).abs().max()) <= 1e-12
    means, scales, rots, vm, _ = (t.double() for t in C.make_geometry(C.GEOMETRY_CASES[-1]))
    q = rots / rots.norm(dim=1, keepdim=True)
    unflipped = C.geometry(means, scales, q, vm)[:, :3]
    k = scales.argmin(1)
    r, x, y, z = q.unbind(1)
    col = torch.stack([torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y + r * z), 2 * (x * z - r * y)], 1),
                       torch.stack([2 * (x * y - r * z), 1 - 2 * (x * x + z * z), 2 * (y * z + r * x)], 1),
                       torch.stack([2 * (x * z + r * y), 2 * (y * z - r * x), 1 - 2 * (x * x + y * y)], 1)], 1)
    n_v = col[torch.arange(len(k)), k] @ vm[:3, :3]
    flipped = ((n_v - unflipped).abs().sum(1) > 1e-9).double().mean()
    assert 0.35 <= float(flipped) <= 0.65
    assert float(((n_v.abs() - unflipped.abs()).abs()).max()) <= 1e-12
