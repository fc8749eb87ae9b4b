"""Per-Gaussian feature channels, the parts that need no GPU: the side struct gsr_features_ext in the header and in
ctypes, its struct_size versioning, the two new entry points and the scratch-size function, the unchanged version-3
ABI, every argument refusal before any device call or allocation, the Python validation errors, and the chunked
oracle truth's self-check."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from gaussian_splatting_lightning_amd import _native
from tests import feature_cases as F
from tests.helpers import run_oracle, settings_for

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gsrast.h")
FIELDS = ("struct_size", "C", "features", "out_features", "dL_dout_features", "dL_dfeatures")
f32 = np.float32


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_features_ext_matches_the_header():
    E = _native.FeaturesExt
    assert tuple(n for n, _ in E._fields_) == FIELDS
    # LP64: the size word, the channel count padded to the pointers' alignment, four pointers
    assert [getattr(E, n).offset for n in FIELDS] == [0, 8, 16, 24, 32, 40] and ctypes.sizeof(E) == 48
    assert E.C.size == ctypes.sizeof(ctypes.c_int)
    assert E().struct_size == ctypes.sizeof(E)  # the constructor fills the size the caller was built with
    body = re.search(r"typedef struct gsr_features_ext \{(.*?)\} gsr_features_ext;", _header(), flags=re.S).group(1)
    assert tuple(re.findall(r"\*?\s*(\w+)\s*;", body)) == FIELDS
    assert _native.FEATURES_MAX_C == 64


def test_entry_points_and_unchanged_abi():
    lib = _native.load()
    for name in ("gsr_forward_features", "gsr_backward_features"):
        assert name in _native.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert re.search(r"\bint " + name + r"\(", _header()), name
    assert "gsr_bwd_scratch_bytes_features" in _native.EXPORTED_SYMBOLS
    assert re.search(r"\bsize_t gsr_bwd_scratch_bytes_features\(", _header())
    assert lib.gsr_abi_version() == _native.ABI_VERSION == 3
    assert re.search(r"#define GSR_ABI_VERSION 3\b", open(HEADER).read())
    # the argument structs and the two earlier side structs are what they were
    assert ctypes.sizeof(_native.ForwardArgs) == 176 and ctypes.sizeof(_native.BackwardArgs) == 368
    assert ctypes.sizeof(_native.CompositeExt) == 48 and ctypes.sizeof(_native.AbsgradExt) == 24


def test_scratch_size_arithmetic():
    lib = _native.load()
    up = lambda n: (n + 255) // 256 * 256  # noqa: E731
    for R, nb in ((0, 0), (1000, 10), (123457, 3), (4_200_000, 1500)):
        base = up(max(R, 1) * 40) + up(max(nb, 1) * 40) + 256
        assert lib.gsr_bwd_scratch_bytes(R, nb) == base  # the plain layout is unchanged
        # the abs layout and the feature layout both start with the plain layout: each is the plain size, which keeps
        # what follows 256-B aligned, plus its own per-instance and per-big-Gaussian rows
        assert base % 256 == 0
        assert lib.gsr_bwd_scratch_bytes_abs(R, nb) == base + up(max(R, 1) * 8) + up(max(nb, 1) * 8)
        for C in (1, 3, 7, 8, 9, 16, 17, 33, 64):
            B = 8 if C <= 8 else 16  # one channel block's rows, whatever C is
            assert lib.gsr_bwd_scratch_bytes_features(R, nb, C) == base + up(max(R, 1) * B * 4) + up(max(nb, 1) * B * 4)
        for C in (0, -1, 65):
            assert lib.gsr_bwd_scratch_bytes_features(R, nb, C) == 0
    # at 4.2 M instances the feature rows are 64 B per instance: 0.27 GB for any C > 8 (per-channel-block processing)
    assert lib.gsr_bwd_scratch_bytes_features(4_200_000, 0, 32) - lib.gsr_bwd_scratch_bytes(4_200_000, 0) < 0.3e9


def _calls():
    """(forward(feat, ext=None, absgrad=None, **args), backward(...)) on a scene whose every other argument is valid:
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

    def fwd(feat, **extra):
        a = _native.ForwardArgs(**{**scene, "out_color": 1, **extra})
        rc = lib.gsr_forward_features(ctypes.byref(a), None, None if feat is None else ctypes.byref(feat), cb, None,
                                      None, ctypes.byref(num))
        return rc, lib.gsr_last_error().decode(), list(asked)

    def bwd(feat, absgrad=None, **extra):
        b = _native.BackwardArgs(**{**scene, "dL_dpix": 1, "geom_buffer": 1, "image_buffer": 1, "dL_dsh": 1, **extra})
        rc = lib.gsr_backward_features(ctypes.byref(b), None, None if absgrad is None else ctypes.byref(absgrad),
                                       None if feat is None else ctypes.byref(feat), cb, None, None)
        return rc, lib.gsr_last_error().decode(), list(asked)

    return fwd, bwd


def test_invalid_arguments_fail_before_touching_the_device():
    fwd, bwd = _calls()
    ok = dict(features=1, out_features=1, dL_dout_features=1, dL_dfeatures=1)
    for C in (0, -3, 65):
        for rc, msg, asked in (fwd(_native.FeaturesExt(C=C, **ok)), bwd(_native.FeaturesExt(C=C, **ok))):
            assert rc == 1 and "C must be" in msg and asked == [], (C, rc, msg)
    for rc, msg, asked in (fwd(_native.FeaturesExt(C=4, out_features=1)), bwd(_native.FeaturesExt(C=4, dL_dfeatures=1))):
        assert rc == 1 and "features is required" in msg and asked == []
    rc, msg, asked = fwd(_native.FeaturesExt(C=4, features=1))
    assert rc == 1 and "out_features" in msg and asked == []
    # struct_size ends before the first pointer field (nothing, the size word alone, C alone, a part of the pointer)
    for size in (0, 8, 16, 23):
        feat = _native.FeaturesExt(C=4, **ok)
        feat.struct_size = size
        for rc, msg, asked in (fwd(feat), bwd(feat)):
            assert rc == 1 and "struct_size" in msg and asked == [], size
    # the plain entry points' own checks are reached through the new ones
    rc, msg, asked = bwd(_native.FeaturesExt(C=4, **ok), P=-1)
    assert rc == 1 and "P must be" in msg and asked == []
    rc, msg, asked = fwd(None, P=-1)
    assert rc == 1 and "P must be" in msg and asked == []


def test_struct_size_versioning():
    """A field the caller's struct_size does not cover whole reads as NULL: seen through which check fires first."""
    fwd, bwd = _calls()
    feat = _native.FeaturesExt(C=4, features=1, out_features=1)
    feat.struct_size = _native.FeaturesExt.out_features.offset  # ends before out_features: NULL
    rc, msg, _ = fwd(feat)
    assert rc == 1 and "out_features" in msg
    feat.struct_size = _native.FeaturesExt.out_features.offset + 4  # covered in part: not there
    rc, msg, _ = fwd(feat)
    assert rc == 1 and "out_features" in msg
    # a backward struct that ends before dL_dout_features carries no upstream gradient: with the absolute sums it is
    # still refused (the check is on the struct, not on the gradient), without them it goes on to the common checks
    feat = _native.FeaturesExt(C=4, features=1, out_features=1, dL_dout_features=1, dL_dfeatures=1)
    feat.struct_size = _native.FeaturesExt.dL_dout_features.offset
    rc, msg, _ = bwd(feat, P=-1)
    assert rc == 1 and "P must be" in msg


def test_unsupported_combinations_are_refused_before_touching_the_device():
    fwd, bwd = _calls()
    ok = dict(features=1, out_features=1, dL_dout_features=1, dL_dfeatures=1)
    rc, msg, asked = bwd(_native.FeaturesExt(C=4, **ok), absgrad=_native.AbsgradExt(dL_dmeans2D_abs=1))
    assert rc == 5 and "dL_dmeans2D_abs" in msg and asked == []
    for stages in (_native.GSR_BWD_COMPOSITE, _native.GSR_BWD_GAUSSIANS):
        rc, msg, asked = bwd(_native.FeaturesExt(C=4, **ok), stages=stages, bwd_scratch=1)
        assert rc == 5 and "stages" in msg and asked == []
    # an absgrad struct without the output pointer asks for nothing: not refused (P = -1 is the error behind)
    rc, msg, _ = bwd(_native.FeaturesExt(C=4, **ok), absgrad=_native.AbsgradExt(), P=-1)
    assert rc == 1 and "P must be" in msg


def _cpu_state(P=4, C=None):
    from gaussian_splatting_lightning_amd.rasterizer import ForwardState
    e = torch.empty(0, dtype=torch.uint8)
    return ForwardState(torch.zeros(P, 3), None, torch.zeros(P, 3), torch.zeros(P, 1), torch.zeros(P, 3),
                        torch.zeros(P, 4), None, torch.zeros(P, dtype=torch.int32), torch.zeros(3), torch.eye(4),
                        torch.eye(4), torch.zeros(3), e, e, e, 0, 0, 0, None if C is None else torch.zeros(P, C))


def test_forward_state_appends_the_features():
    from gaussian_splatting_lightning_amd.rasterizer import ForwardState
    assert ForwardState._fields[-1] == "features" and ForwardState._fields[15:18] == ("num_rendered", "num_big", "M")
    assert _cpu_state().features is None  # the 18-field construction of earlier callers still works
    assert len(_cpu_state()[:15]) == 15 and all(torch.is_tensor(t) or t is None for t in _cpu_state()[:15])


def test_python_argument_validation():
    from gaussian_splatting_lightning_amd import GaussianRasterizer, rasterize_gaussians
    from gaussian_splatting_lightning_amd.rasterizer import _features, backward_chunked, backward_raw
    dev = torch.device("cpu")
    inp = F.scene("A")[0]
    rs = settings_for(inp, dev)
    for bad, what in ((torch.zeros(4), "shape"), (torch.zeros(5, 3), "shape"), (torch.zeros(4, 3, 1), "shape"),
                      (torch.zeros(4, 0), "between 1 and 64"), (torch.zeros(4, 65), "between 1 and 64"),
                      (torch.zeros(4, 3, dtype=torch.float64), "float32"), ("x", "shape")):
        with pytest.raises(RuntimeError, match=what):
            _features(bad, 4, dev)
    t = torch.zeros(7, 4)[:, 1:]  # a non-contiguous view becomes a contiguous (P,C) tensor
    assert _features(t, 4 + 3, dev).is_contiguous() and _features(t, 7, dev).shape == (7, 3)
    st = _cpu_state(C=5)
    with pytest.raises(RuntimeError, match="grad_out_features must have shape"):
        backward_raw(st, rs, None, grad_out_features=torch.zeros(4, rs.image_height, rs.image_width))
    with pytest.raises(RuntimeError, match="features"):
        backward_raw(st, rs, None, out={"features": torch.zeros(4, 4)})
    with pytest.raises(RuntimeError, match="needs a state"):
        backward_raw(_cpu_state(), rs, None, grad_out_features=torch.zeros(5, rs.image_height, rs.image_width))
    with pytest.raises(NotImplementedError, match="features"):
        backward_chunked(st, rs, None, None, [(0, 4, {})])
    z = torch.zeros(4, 3)
    with pytest.raises(NotImplementedError, match="absgrad"):
        rasterize_gaussians(z, None, None, z, torch.zeros(4, 1), z, torch.zeros(4, 4), None, rs, absgrad=True,
                            features=torch.zeros(4, 2))
    with pytest.raises(NotImplementedError, match="absgrad"):
        GaussianRasterizer(rs, absgrad=True)(z, None, torch.zeros(4, 1), colors_precomp=z, scales=z,
                                             rotations=torch.zeros(4, 4), features=torch.zeros(4, 2))


def test_chunked_truth_of_three_channels_is_one_oracle_call():
    for name in ("A", "B"):
        inp = F.scene(name)[0]
        f, dF = F.inputs(name, 3)
        t = F.truth(name, 3)
        color, _, _, run = run_oracle(dict(inp, bg=np.zeros(3, f32)), colors_precomp=f)
        g = run.backward(dF, None)
        assert np.array_equal(t["image"].view(np.uint32), color.view(np.uint32))
        assert np.array_equal(t["features"].view(np.uint32), g["colors"].view(np.uint32))
        for k in F.GEOMETRY:
            assert t[k].dtype == np.float64 and np.array_equal(t[k], g[k].astype(np.float64)), k
        assert t["flip_candidates"] == 0
    # zero-padding the last chunk: channel 6 of C = 7 is a one-channel oracle call's channel 0
    t7 = F.truth("A2", 7)
    img, flips, g = F.chunk_truth(F.scene("A2")[0], F.inputs("A2", 7)[0][:, 6:7], F.inputs("A2", 7)[1][6:7])
    assert np.array_equal(t7["image"][6].view(np.uint32), img[0].view(np.uint32)) and flips == 0
    assert np.array_equal(t7["features"][:, 6], g["colors"][:, 0]) and t7["flip_candidates"] == 0
    assert int(np.count_nonzero(np.abs(t7["features"]).sum(1))) == 463  # Gaussians with a feature gradient (of 600)
