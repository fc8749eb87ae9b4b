"""The median depth map, the parts that need no GPU: the side struct gsr_median_ext in the header and in ctypes, the
new entry points (the rasterizer's two and the three of the blended-surface normals), the unchanged version-3 ABI,
every argument refusal before any device call or allocation, the dispatchers' choice of entry point, the Python
validation errors and output order, and the fixture's regeneration on scene A with the census the tests rely on."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from gaussian_splatting_lightning_amd import _native
from tests import absgrad_cases as AC
from tests import distortion_cases as DC
from tests import median_cases as MC
from tests.helpers import settings_for

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gsrast.h")
FIELDS = ("struct_size", "out_median_depth", "out_median_index", "median_pos", "dL_dmedian_depth")
SURFACE = ("gsr_normal_consistency_forward_surface", "gsr_depth_to_normal_surface",
           "gsr_normal_consistency_backward_surface")
f32, f64 = np.float32, np.float64


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_median_ext_matches_the_header():
    E = _native.MedianExt
    assert tuple(n for n, _ in E._fields_) == FIELDS
    assert [getattr(E, n).offset for n in FIELDS] == [0, 8, 16, 24, 32] and ctypes.sizeof(E) == 40  # LP64
    assert E().struct_size == ctypes.sizeof(E)  # the constructor fills the size the caller was built with
    body = re.search(r"typedef struct gsr_median_ext \{(.*?)\} gsr_median_ext;", _header(), flags=re.S).group(1)
    assert tuple(re.findall(r"\*?\s*(\w+)\s*;", body)) == FIELDS


def test_entry_points_and_unchanged_abi():
    lib = _native.load()
    for name in ("gsr_forward_median", "gsr_backward_median") + SURFACE:
        assert name in _native.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert re.search(r"\bint " + name + r"\(", _header()), name
        assert getattr(lib, name).restype is ctypes.c_int
    assert lib.gsr_abi_version() == _native.ABI_VERSION == 3  # new entry points, not a new ABI
    assert re.search(r"#define GSR_ABI_VERSION 3\b", open(HEADER).read())
    # the argument structs and the four earlier side structs are what they were
    assert ctypes.sizeof(_native.ForwardArgs) == 176 and ctypes.sizeof(_native.BackwardArgs) == 368
    assert ctypes.sizeof(_native.CompositeExt) == 48 and ctypes.sizeof(_native.AbsgradExt) == 24
    assert ctypes.sizeof(_native.FeaturesExt) == 48 and ctypes.sizeof(_native.DistortionExt) == 56
    names = [lib.gsr_stage_name(i).decode() for i in range(lib.gsr_num_stages())]
    assert "median_fwd" in names and "median_bwd" in names
    assert names[-2:] == ["contrib_walk", "contrib_gather"] and len(names) == len(set(names))
    # the backward needs no scratch of its own: the sizes are what they were
    assert lib.gsr_bwd_scratch_bytes(1000, 10) == 40192 + 512 + 256


def _calls():
    """(forward(med, **args), backward(med, absgrad=None, **args)) on a scene whose every other argument is valid:
    return (code, message, allocations asked for).  On a host without a GPU a device call would give GSR_ERR_HIP (2)."""
    lib = _native.load()
    asked = []

    def alloc(_ctx, which, nbytes):
        asked.append((which, nbytes))
        return None

    cb = _native.ALLOC_FN(alloc)
    scene = dict(P=5, W=10, H=10, D=0, M=1, means3D=1, opacities=1, viewmatrix=1, projmatrix=1, shs=1, campos=1,
                 scales=1, rotations=1, radii=1, background=1)
    num = ctypes.c_int64(0)
    ref = lambda s: None if s is None else ctypes.byref(s)  # noqa: E731

    def fwd(med, dist=None, **extra):
        a = _native.ForwardArgs(**{**scene, "out_color": 1, **extra})
        rc = lib.gsr_forward_median(ctypes.byref(a), None, None, ref(dist), ref(med), cb, None, None,
                                    ctypes.byref(num))
        return rc, lib.gsr_last_error().decode(), list(asked)

    def bwd(med, absgrad=None, dist=None, **extra):
        b = _native.BackwardArgs(**{**scene, "dL_dpix": 1, "geom_buffer": 1, "image_buffer": 1, "dL_dsh": 1, **extra})
        rc = lib.gsr_backward_median(ctypes.byref(b), None, ref(absgrad), None, ref(dist), ref(med), cb, None, None)
        return rc, lib.gsr_last_error().decode(), list(asked)

    return fwd, bwd


OK = dict(out_median_depth=1, out_median_index=1, median_pos=1, dL_dmedian_depth=1)


def test_invalid_arguments_fail_before_touching_the_device():
    fwd, bwd = _calls()
    E = _native.MedianExt
    for missing in ("out_median_depth", "out_median_index"):
        rc, msg, asked = fwd(E(**{k: v for k, v in OK.items() if k != missing}))
        assert rc == 1 and "out_median_depth and out_median_index" in msg and asked == [], (missing, rc, msg)
    for call in (fwd, bwd):
        rc, msg, asked = call(E(**{k: v for k, v in OK.items() if k != "median_pos"}))
        assert rc == 1 and "median_pos" in msg and asked == [], (rc, msg)
    # the backward reads neither output plane
    rc, msg, asked = bwd(E(median_pos=1, dL_dmedian_depth=1), P=-1)
    assert rc == 1 and "P must be" in msg and asked == []
    # struct_size ends before the first pointer field (nothing, the size word alone, a part of the pointer)
    for size in (0, 8, 15):
        m = E(**OK)
        m.struct_size = size
        for rc, msg, asked in (fwd(m), bwd(m)):
            assert rc == 1 and "struct_size" in msg and asked == [], size
    # the plain entry points' own checks are reached through the new ones, and the distortion struct's come first
    rc, msg, asked = fwd(E(**OK), P=-1)
    assert rc == 1 and "P must be" in msg and asked == []
    rc, msg, asked = fwd(None, P=-1)
    assert rc == 1 and "P must be" in msg and asked == []
    bad = _native.DistortionExt(map=7, out_distortion=1, total_weight=1, total_moment=1)
    for rc, msg, asked in (fwd(E(**OK), dist=bad), bwd(E(**OK), dist=bad)):
        assert rc == 1 and "map must be" in msg and asked == []
    # the blended-surface normals: a null median, a ratio that is not finite, a bad shape
    lib = _native.load()
    img = (4, 5, 0.5, 0.5)
    assert lib.gsr_normal_consistency_forward_surface(*img, 1, 1, 1, None, 0.5, 1, None, None) == 1
    assert "null array" in lib.gsr_last_error().decode()
    assert lib.gsr_depth_to_normal_surface(*img, 1, 1, None, 0.5, 1, None) == 1
    assert lib.gsr_normal_consistency_backward_surface(*img, 1, 1, 1, 1, 0.5, 1, 1, 1, 1, None, None) == 1
    for r in (float("nan"), float("inf")):
        assert lib.gsr_normal_consistency_forward_surface(*img, 1, 1, 1, 1, r, 1, None, None) == 1
        assert "depth_ratio" in lib.gsr_last_error().decode()
        assert lib.gsr_depth_to_normal_surface(*img, 1, 1, 1, r, 1, None) == 1
        assert lib.gsr_normal_consistency_backward_surface(*img, 1, 1, 1, 1, r, 1, 1, 1, 1, 1, None) == 1
    assert lib.gsr_normal_consistency_forward_surface(0, 5, 0.5, 0.5, 1, 1, 1, 1, 0.5, 1, None, None) == 1


def test_unsupported_combinations_are_refused_before_touching_the_device():
    fwd, bwd = _calls()
    E = _native.MedianExt
    rc, msg, asked = bwd(E(**OK), absgrad=_native.AbsgradExt(dL_dmeans2D_abs=1))
    assert rc == 5 and "dL_dmeans2D_abs" in msg and asked == []
    for stages in (_native.GSR_BWD_COMPOSITE, _native.GSR_BWD_GAUSSIANS):
        rc, msg, asked = bwd(E(**OK), stages=stages, bwd_scratch=1)
        assert rc == 5 and "stages" in msg and asked == []
    # together with the distortion map: not refused (P = -1 is the error behind)
    dist = _native.DistortionExt(map=0, out_distortion=1, total_weight=1, total_moment=1, dL_ddistortion=1)
    rc, msg, _ = bwd(E(**OK), dist=dist, P=-1)
    assert rc == 1 and "P must be" in msg


class _Lib:
    """Records which entry point a dispatcher reaches, and with which side structs."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, sum(a is not None and not isinstance(a, int) for a in args)))
            return 0
        return entry


def test_dispatchers_pick_the_narrowest_entry_point():
    fa, ba, num = _native.ForwardArgs(), _native.BackwardArgs(), ctypes.c_int64(0)
    ext, feat = _native.CompositeExt(), _native.FeaturesExt()
    dist, med, ab = _native.DistortionExt(), _native.MedianExt(), _native.AbsgradExt()
    lib = _Lib()
    for kw, want in ((dict(), "gsr_forward"), (dict(ext=ext), "gsr_forward_ext"),
                     (dict(feat=feat), "gsr_forward_features"), (dict(dist=dist), "gsr_forward_distortion"),
                     (dict(median=med), "gsr_forward_median"), (dict(dist=dist, median=med), "gsr_forward_median")):
        _native.call_forward(lib, fa, kw.get("ext"), kw.get("feat"), None, None, num, dist=kw.get("dist"),
                             median=kw.get("median"))
        assert lib.calls[-1][0] == want, kw
    for kw, want in ((dict(), "gsr_backward"), (dict(ext=ext), "gsr_backward_ext"), (dict(absgrad=ab), "gsr_backward_abs"),
                     (dict(feat=feat), "gsr_backward_features"), (dict(dist=dist), "gsr_backward_distortion"),
                     (dict(median=med), "gsr_backward_median"), (dict(feat=feat, median=med), "gsr_backward_median")):
        _native.call_backward(lib, ba, kw.get("ext"), kw.get("absgrad"), kw.get("feat"), None, None,
                              dist=kw.get("dist"), median=kw.get("median"))
        assert lib.calls[-1][0] == want, kw


def _cpu_state(P=4, median=False):
    from gaussian_splatting_lightning_amd.rasterizer import ForwardState, MedianState, _DistortionForwardState
    e = torch.empty(0, dtype=torch.uint8)
    fields = (torch.zeros(P, 3), None, torch.zeros(P, 3), torch.zeros(P, 1), torch.zeros(P, 3), torch.zeros(P, 4),
              None, torch.zeros(P, dtype=torch.int32), torch.zeros(3), torch.eye(4), torch.eye(4), torch.zeros(3), e, e,
              e, 0, 0, 0)
    if not median:
        return ForwardState(*fields)
    st = _DistortionForwardState(*fields)
    st.median = MedianState(torch.full((24, 40), -1, dtype=torch.int32))
    return st


def test_python_argument_validation_and_output_order(monkeypatch):
    import gaussian_splatting_lightning_amd.rasterizer as R
    from gaussian_splatting_lightning_amd import GaussianRasterizer, normal_consistency, rasterize_gaussians
    from gaussian_splatting_lightning_amd import depth_to_normal, render_normal_consistency
    inp = MC.scene("A")
    rs = settings_for(inp, torch.device("cpu"))
    H, W = rs.image_height, rs.image_width
    z = torch.zeros(4, 3)
    with pytest.raises(NotImplementedError, match="absgrad"):
        rasterize_gaussians(z, None, None, z, torch.zeros(4, 1), z, torch.zeros(4, 4), None, rs, absgrad=True,
                            median_depth=True)
    assert GaussianRasterizer(rs, median_depth=True).median_depth and not GaussianRasterizer(rs).median_depth
    # the state: ForwardState's fields are what they were, the median rides on the subclass as an attribute
    st = _cpu_state(median=True)
    assert isinstance(st, R.ForwardState) and len(st) == len(R.ForwardState._fields) == 19
    assert st.median.pos.shape == (H, W) and st.distortion is None
    assert getattr(_cpu_state(), "median", None) is None
    with pytest.raises(RuntimeError, match="grad_out_median_depth must have shape"):
        R.backward_raw(st, rs, None, grad_out_median_depth=torch.zeros(1, H, W + 1))
    with pytest.raises(RuntimeError, match="needs a state"):
        R.backward_raw(_cpu_state(), rs, None, grad_out_median_depth=torch.zeros(1, H, W))
    with pytest.raises(NotImplementedError, match="median"):
        R.backward_chunked(st, rs, None, None, [(0, 4, {})])
    # the output order, with the library call replaced: (..., alpha, features, distortion, median_depth, median_index)
    seen = {}

    def fake_forward(lib, a, ext, feat, cb, stream, num_rendered, dist=None, median=None):
        seen.update(ext=ext, feat=feat, dist=dist, median=median)
        return 0

    class Dev:  # a tensor that claims a HIP device
        type = "cuda"
    monkeypatch.setattr(_native, "call_forward", fake_forward)
    monkeypatch.setattr(_native, "load", lambda: None)
    monkeypatch.setattr(R, "_stream_handle", lambda d: None)
    monkeypatch.setattr(torch.cuda, "device", lambda d: __import__("contextlib").nullcontext())
    real_empty = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *s, device=None, **kw: real_empty(*s, **kw))
    monkeypatch.setattr(R, "_prep", lambda t, device, name: None if t is None or t.numel() == 0 else t.contiguous())
    monkeypatch.setattr(R, "_features", lambda f, P, device: f)

    class Means(torch.Tensor):
        @property
        def device(self):
            return Dev()
    means = torch.zeros(4, 3).as_subclass(Means)
    args = (means, None, z, torch.zeros(4, 1), z, torch.zeros(4, 4), None, rs)
    res = R.forward_raw(*args, return_alpha=True, features=torch.zeros(4, 5), distortion="z", median_depth=True)
    assert [tuple(t.shape) for t in res[:-1]] == [(3, H, W), (4,), (1, H, W), (1, H, W), (5, H, W), (1, H, W),
                                                  (1, H, W), (1, H, W)]
    assert res[-3].dtype == torch.float32 and res[-2].dtype == torch.int32
    assert isinstance(seen["median"], _native.MedianExt) and seen["median"].dL_dmedian_depth is None
    assert res[-1].median.pos.shape == (H, W) and res[-1].distortion.map == "z"
    res = R.forward_raw(*args, median_depth=True)
    assert len(res) == 6 and seen["dist"] is None and seen["ext"] is None and seen["median"] is not None
    res = R.forward_raw(*args)
    assert len(res) == 4 and seen["median"] is None and type(res[-1]) is R.ForwardState
    monkeypatch.undo()
    # the surface normals' argument checks come before any device work
    img = torch.zeros(1, H, W)
    with pytest.raises(ValueError):  # (the images are checked first: not on the device)
        normal_consistency(img, img, torch.zeros(3, H, W), rs, depth_ratio=0.5)
    with pytest.raises(ValueError):
        depth_to_normal(img, img, rs, median_depth=torch.zeros(1, H, W + 1), depth_ratio=1.0)
    from gaussian_splatting_lightning_amd import normals as NM
    assert NM._surface_args("x", rs, None, 0.0) == (0.0, False)
    with pytest.raises(ValueError, match="depth_ratio must be finite"):
        NM._surface_args("x", rs, img, float("nan"))
    with pytest.raises(ValueError, match="needs median_depth"):
        NM._surface_args("x", rs, None, 0.5)
    with pytest.raises(ValueError, match=r"median_depth \(1,"):
        NM._surface_args("x", rs, torch.zeros(H, W), 0.5)
    with pytest.raises(ValueError, match="median_depth=True"):
        render_normal_consistency(GaussianRasterizer(rs, return_alpha=True), z, None, torch.zeros(4, 1), shs=None,
                                  scales=z, rotations=torch.zeros(4, 4), depth_ratio=1.0)


def test_scene_A_truth_regenerates_to_the_fixture():
    t, fx = MC.truth("A"), MC.fixture_truth("A")
    assert set(t) | {"g_sha256"} == set(fx)
    for k in ("index", "depth", "z", "candidate", "adjacent", "last"):
        assert t[k].dtype == fx[k].dtype and np.array_equal(t[k].view(np.uint8), fx[k].view(np.uint8)), k
    for k in ("dz", "means3D"):
        assert t[k].dtype == f64 and np.allclose(t[k], fx[k], rtol=1e-12, atol=0), k
    for k in ("longest", "max_distinct", "flip_candidates"):
        assert int(t[k]) == int(fx[k]), k
    assert np.isclose(t["closest"], fx["closest"], rtol=1e-6) and float(t["margin"]) == float(fx["margin"])
    for k in ("err_dz", "err_means3D"):  # (a float32 restatement's error: a last-place difference moves it)
        assert np.isclose(t[k], fx[k], rtol=1e-3), k


def test_census_of_the_scenes():
    """What the GPU tests rely on, from the fixture: the margin's derivation, the candidate fraction, the pixels whose
    median is the last contributor, scene A's untouched pixels and its tile with many distinct medians."""
    want = dict(A=(218, 12, 0), A2=(16, 0, 0), B=(51, 0, 5))
    for name in MC.SCENES:
        t = MC.fixture_truth(name)
        n, W, H = AC.SCENES[name][:3]
        assert float(t["margin"]) == MC.margin(int(t["longest"])) == int(t["longest"]) * 2.0 ** -23 * 4.0
        cand = int(t["candidate"].sum())
        assert (int(t["last"].sum()), int((t["index"] < 0).sum()), cand) == want[name], name
        assert cand <= MC.MAX_CANDIDATE_FRACTION * W * H and int(t["flip_candidates"]) == 0
        assert (cand == 0) == (float(t["closest"]) > float(t["margin"]))
        on = t["index"] >= 0
        assert np.array_equal(t["depth"][on].view(np.uint32), t["z"][t["index"][on]].view(np.uint32))
        assert np.all(t["depth"][~on] == 0) and np.all(t["adjacent"][~t["candidate"]] == t["index"][~t["candidate"], None])
        assert np.all((t["adjacent"][t["candidate"]] == t["index"][t["candidate"], None]).any(-1))
        assert not MC.upstream(name)[0][t["candidate"]].any() and MC.upstream(name)[0][~t["candidate"]].all()
        assert np.count_nonzero(t["dz"]) == np.unique(t["index"][on & ~t["candidate"]]).size
    assert int(MC.fixture_truth("A")["max_distinct"]) == 71  # a quadratic segmented sum would show here


def test_median_of_a_list():
    """The rule on hand-made lists: the last contributor whose incoming transmittance exceeds 1/2."""
    w = lambda *a: np.asarray(a, f32)  # noqa: E731
    assert MC.pixel_median(w())[0] == -1
    assert MC.pixel_median(w(0.2))[0] == 0 and MC.pixel_median(w(0.9))[0] == 0
    assert MC.pixel_median(w(0.3, 0.3, 0.2))[0] == 1   # incoming 1, 0.7, 0.4
    assert MC.pixel_median(w(0.1, 0.1, 0.1))[0] == 2   # never half opaque: the last
    assert MC.pixel_median(w(0.5, 0.25))[0] == 0       # incoming exactly 0.5 does not exceed it
    # the restated float32 sum agrees with the float64 truth to its stored error
    t = MC.fixture_truth("B")
    dz32, m32 = MC.restated("B", t["index"], MC.upstream("B"))
    assert np.isclose(np.linalg.norm(m32.astype(f64) - t["means3D"]), float(t["err_means3D"]), rtol=1e-3)
    # the blended surface: ratio 0 is the expected-depth restatement of tests/normal_cases.py
    from tests import normal_cases as NC
    case = MC.SURFACE_CASES[1]
    D, A, N, M, dE = (x.double() for x in MC.make_surface(case))
    assert torch.equal(MC.surface_consistency(D, A, N, M, 0.0, case.tanfovx, case.tanfovy),
                       NC.consistency(D, A, N, case.tanfovx, case.tanfovy))
    assert not torch.equal(MC.surface_consistency(D, A, N, M, 1.0, case.tanfovx, case.tanfovy),
                           NC.consistency(D, A, N, case.tanfovx, case.tanfovy))
