"""Per-Gaussian contribution statistics (gsr_contributions), the parts that need no GPU: the two exported symbols, the
argument struct in the header and in ctypes with its struct_size versioning, the scratch-size function, every argument
refusal before any device call or allocation, the Python validation errors, and the fixture's truth of scene A
regenerated from the oracle."""
import ctypes
import hashlib
import os
import re
import types

import numpy as np
import pytest
import torch

from gaussian_splatting_lightning_amd import _native
from tests import absgrad_cases as AC
from tests import contrib_cases as CC
from tests.helpers import load_golden, settings_for

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gsrast.h")
FIELDS = ("struct_size", "P", "W", "H", "R", "num_big", "radii", "geom_buffer", "binning_buffer", "image_buffer",
          "pixel_weights", "count", "wsum", "wmax", "accumulate")
GSR_ERR_ARG = 1


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_library_exports_the_entry_points():
    lib = _native.load()
    for name, ret in (("gsr_contributions", "int"), ("gsr_contrib_scratch_bytes", "size_t")):
        assert name in _native.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert re.search(r"\b" + ret + " " + name + r"\(", _header()), name
    assert hasattr(lib, "gsr_densify_classify_keep")
    assert lib.gsr_abi_version() == _native.ABI_VERSION == 3  # a new entry point, not a new ABI
    assert ctypes.sizeof(_native.ForwardArgs) == 176 and ctypes.sizeof(_native.BackwardArgs) == 368
    names = [lib.gsr_stage_name(i).decode() for i in range(lib.gsr_num_stages())]
    assert names[-2:] == ["contrib_walk", "contrib_gather"] and names[-3] == "feat_gather"


def test_contrib_args_match_the_header():
    A = _native.ContribArgs
    assert tuple(n for n, _ in A._fields_) == FIELDS
    body = re.search(r"typedef struct gsr_contrib_args \{(.*?)\} gsr_contrib_args;", _header(), flags=re.S).group(1)
    declared = []
    for stmt in body.split(";"):  # "int P, W, H" / "const void *geom_buffer, *binning_buffer, *image_buffer"
        stmt = stmt.strip()
        if stmt:
            first, *more = stmt.split(",")
            declared += [re.search(r"(\w+)\s*$", first).group(1)] + [m.strip().lstrip("*").strip() for m in more]
    assert tuple(declared) == FIELDS
    # LP64: the size word, three ints and four bytes of padding, two int64, eight pointers, an int (padded)
    want = [0, 8, 12, 16, 24, 32] + [40 + 8 * k for k in range(8)] + [104]
    assert [getattr(A, n).offset for n in FIELDS] == want and ctypes.sizeof(A) == 112
    assert A.count.size == 8 and A.R.size == 8 and A.accumulate.size == ctypes.sizeof(ctypes.c_int)
    assert A().struct_size == ctypes.sizeof(A)  # the constructor fills the size the caller was built with


def test_scratch_size():
    lib = _native.load()
    up = lambda n: (n + 255) // 256 * 256  # noqa: E731
    assert lib.gsr_contrib_scratch_bytes(0, 0) > 0
    for R, nb in ((0, 0), (1, 1), (1000, 10), (123457, 3), (4_200_000, 1500)):
        assert lib.gsr_contrib_scratch_bytes(R, nb) == up(max(R, 1) * 16) + up(max(nb, 1) * 16)  # 16-B rows
    sizes = [lib.gsr_contrib_scratch_bytes(R, 7) for R in (0, 1, 16, 17, 1000, 10**6, 10**7)]
    assert sizes == sorted(sizes) and sizes[-1] > sizes[0]
    sizes = [lib.gsr_contrib_scratch_bytes(10**6, nb) for nb in (0, 1, 16, 17, 1000, 15000)]
    assert sizes == sorted(sizes) and sizes[-1] > sizes[0]
    # num_big unknown on the host (< 0): room for the most there can be
    assert lib.gsr_contrib_scratch_bytes(10**6, -1) >= lib.gsr_contrib_scratch_bytes(10**6, 10**6 // 65)


def _call(**fields):
    """gsr_contributions on arguments that are valid unless `fields` says otherwise: (code, message, allocations asked
    for).  On a host without a GPU a device call would give GSR_ERR_HIP (2)."""
    lib = _native.load()
    asked = []

    def alloc(_ctx, which, nbytes):
        asked.append((which, nbytes))
        return None

    cb = _native.ALLOC_FN(alloc)
    size = fields.pop("struct_size", None)
    ok = dict(P=5, W=10, H=10, R=20, num_big=0, radii=1, geom_buffer=1, binning_buffer=1, image_buffer=1, count=1,
              wsum=1, wmax=1)
    a = _native.ContribArgs(**{**ok, **fields})
    if size is not None:
        a.struct_size = size
    rc = lib.gsr_contributions(ctypes.byref(a), cb, None, None)
    return rc, lib.gsr_last_error().decode(), asked


def test_invalid_arguments_fail_before_any_allocation():
    rc, msg, asked = _call(count=None, wsum=None, wmax=None)
    assert rc == GSR_ERR_ARG and "no output" in msg and asked == []
    for missing in ("radii", "geom_buffer", "binning_buffer", "image_buffer"):
        rc, msg, asked = _call(**{missing: None})
        assert rc == GSR_ERR_ARG and "forward buffers" in msg and asked == [], missing
    # struct_size ends before the first pointer field: nothing, the size word alone, the scalars, a part of the pointer
    for size in (0, 8, 24, 40, 47):
        rc, msg, asked = _call(struct_size=size)
        assert rc == GSR_ERR_ARG and "struct_size" in msg and asked == [], size
    # a struct that ends before the outputs asks for none
    rc, msg, asked = _call(struct_size=_native.ContribArgs.count.offset)
    assert rc == GSR_ERR_ARG and "no output" in msg and asked == []
    for bad, what in ((dict(P=-1), "P must be"), (dict(W=0), "positive"), (dict(R=-1), "num_rendered"),
                      (dict(num_big=6), "num_big")):
        rc, msg, asked = _call(**bad)
        assert rc == GSR_ERR_ARG and what in msg and asked == [], bad
    lib = _native.load()
    assert lib.gsr_contributions(None, _native.ALLOC_FN(lambda c, w, b: None), None, None) == GSR_ERR_ARG
    # no Gaussian: nothing to do, nothing written, no device call, even without forward buffers
    rc, msg, asked = _call(P=0, R=0, radii=None, geom_buffer=None, binning_buffer=None, image_buffer=None)
    assert rc == 0 and asked == []
    # the keep-mask classify checks its arguments likewise
    assert lib.gsr_densify_classify_keep(-1, None, None, 1, None, None) == GSR_ERR_ARG
    assert lib.gsr_densify_classify_keep(5, None, 1, 1, 1, None) == GSR_ERR_ARG
    assert lib.gsr_densify_classify_keep(5, 1, 1, None, 1, None) == GSR_ERR_ARG


def _cpu_state(P=4):
    from gaussian_splatting_lightning_amd.rasterizer import ForwardState
    e = torch.empty(0, dtype=torch.uint8)
    return ForwardState(torch.zeros(P, 3), None, torch.zeros(P, 3), torch.zeros(P, 1), torch.zeros(P, 3),
                        torch.zeros(P, 4), None, torch.zeros(P, dtype=torch.int32), torch.zeros(3), torch.eye(4),
                        torch.eye(4), torch.zeros(3), e, e, e, 0, 0, 0)


def test_python_argument_validation():
    from gaussian_splatting_lightning_amd import GaussianRasterizer, densify, rasterize_contributions
    from gaussian_splatting_lightning_amd.rasterizer import contributions_raw
    dev = torch.device("cpu")
    rs = settings_for(CC.scene("A"), dev)
    H, W = rs.image_height, rs.image_width
    st = _cpu_state()
    for bad, what in ((torch.zeros(W, H), "shape"), (torch.zeros(3, H, W), "shape"), (torch.zeros(H * W), "shape"),
                      (torch.zeros(H, W, dtype=torch.float64), "float32"), (np.zeros((H, W), np.float32), "shape")):
        with pytest.raises(RuntimeError, match=what):
            contributions_raw(st, rs, pixel_weights=bad)
    good = dict(count=torch.zeros(4, dtype=torch.int64), wsum=torch.zeros(4), wmax=torch.zeros(4))
    for name, bad in (("count", torch.zeros(4, dtype=torch.int32)), ("count", torch.zeros(4)),
                      ("wsum", torch.zeros(5)), ("wsum", torch.zeros(4, 1)), ("wmax", torch.zeros(4, dtype=torch.float64)),
                      ("wmax", torch.zeros(8)[::2])):
        with pytest.raises(RuntimeError, match=name):
            contributions_raw(st, rs, out={**good, name: bad})
    with pytest.raises(RuntimeError, match="count, wsum and wmax"):
        contributions_raw(st, rs, out=dict(hits=torch.zeros(4)))
    with pytest.raises(RuntimeError, match="accumulate"):
        contributions_raw(st, rs, accumulate=True)
    # everything valid: the first thing after the checks is the device test (no library call was made before it)
    for kw in (dict(), dict(pixel_weights=torch.zeros(1, H, W)), dict(out=good, accumulate=True)):
        with pytest.raises(RuntimeError, match="HIP device"):
            contributions_raw(st, rs, **kw)
    z = torch.zeros(4, 3)
    with pytest.raises(Exception, match="at most one"):
        rasterize_contributions(z, torch.zeros(4, 1), rs, shs=torch.zeros(4, 1, 3), colors_precomp=z, scales=z,
                                rotations=torch.zeros(4, 4))
    with pytest.raises(Exception, match="scale/rotation pair"):
        GaussianRasterizer(rs).contributions(z, torch.zeros(4, 1), scales=z)
    with pytest.raises(RuntimeError, match="HIP device"):  # neither SHs nor colours: rendered with zero colours
        GaussianRasterizer(rs).contributions(z, torch.zeros(4, 1), scales=z, rotations=torch.zeros(4, 4))
    # the model layer
    g = types.SimpleNamespace(_xyz=torch.zeros(4, 3), contrib_wmax=None)
    for kw in (dict(), dict(threshold=0.1, keep_ratio=0.5)):
        with pytest.raises(RuntimeError, match="exactly one of threshold and keep_ratio"):
            densify.prune_by_contribution(g, "wmax", **kw)
    with pytest.raises(RuntimeError, match="score must be"):
        densify.prune_by_contribution(g, "weight", threshold=0.1)
    with pytest.raises(RuntimeError, match="no accumulated statistics"):
        densify.prune_by_contribution(g, "wmax", threshold=0.1)
    with pytest.raises(RuntimeError, match="shape"):
        densify.prune_by_contribution(g, torch.zeros(5), keep_ratio=0.5)
    with pytest.raises(RuntimeError, match="keep_ratio must be"):
        densify.prune_by_contribution(g, torch.zeros(4), keep_ratio=1.5)
    with pytest.raises(RuntimeError, match="exactly one of stats and rasterizer"):
        densify.accumulate_contributions(g)
    with pytest.raises(RuntimeError, match="stats\\['count'\\]"):
        densify.accumulate_contributions(g, dict(count=torch.zeros(4), wsum=torch.zeros(4), wmax=torch.zeros(4)))
    with pytest.raises(RuntimeError, match="keep_mask"):
        densify.prune_points(g, torch.ones(4))


def test_accumulators_on_the_host():
    """accumulate_contributions with a stats dict is plain tensor arithmetic: the buffers are created lazily, add up
    over views and are dropped by reset_contributions."""
    from gaussian_splatting_lightning_amd import densify
    g = types.SimpleNamespace(_xyz=torch.zeros(3, 3))
    a = dict(count=torch.tensor([1, 0, 5]), wsum=torch.tensor([0.5, 0.0, 2.0]), wmax=torch.tensor([0.5, 0.0, 0.75]))
    b = dict(count=torch.tensor([2, 0, 1]), wsum=torch.tensor([0.25, 0.0, 0.125]), wmax=torch.tensor([0.125, 0.0, 0.875]))
    densify.accumulate_contributions(g, a)
    densify.accumulate_contributions(g, b)
    assert g.contrib_count.dtype == torch.int64 and g.contrib_count.tolist() == [3, 0, 6]
    assert g.contrib_wsum.tolist() == [0.75, 0.0, 2.125] and g.contrib_wmax.tolist() == [0.5, 0.0, 0.875]
    densify.reset_contributions(g)
    assert g.contrib_count is None and g.contrib_wsum is None and g.contrib_wmax is None
    g._xyz = torch.zeros(2, 3)  # another number of Gaussians: fresh buffers
    densify.accumulate_contributions(g, {k: v[:2] for k, v in a.items()})
    assert g.contrib_count.tolist() == [1, 0]


def test_fixture_truth_regenerates():
    """tests/golden/contrib.npz against a fresh oracle truth of scene A, and the fixture's own consistency."""
    z = load_golden("contrib")
    t = CC.truth("A")
    assert CC.flip_candidates("A") == 0
    for k, v in t.items():
        want = z[f"A_{k}"]
        assert want.shape == v.shape == (AC.SCENES["A"][0],) and want.dtype == v.dtype, k
        if k.endswith("count"):
            assert np.array_equal(v, want), k
        else:
            assert np.allclose(v, want, rtol=1e-6, atol=0), k
    for name in CC.SCENES:
        assert int(z[f"{name}_flip_candidates"]) == 0
        assert str(z[f"{name}_weights_sha256"]) == hashlib.sha256(CC.weights(name).tobytes()).hexdigest()
        m = CC.weights(name)
        assert 0.2 < float((m == 0).mean()) < 0.3 and 0 < float((m < 0).mean()) < 0.05
        for pre in ("", "m_"):
            c, s, mx = (z[f"{name}_{pre}{k}"] for k in CC.KINDS)
            assert c.dtype == np.int64 and s.dtype == mx.dtype == np.float64
            assert np.all((c > 0) == (s > 0)) and np.all((c > 0) == (mx > 0))
            assert np.all(mx <= s) and np.all(s <= c * mx * (1 + 1e-12)) and np.all(mx <= 0.99)
        assert np.all(z[f"{name}_m_count"] <= z[f"{name}_count"]) and np.all(z[f"{name}_m_wmax"] <= z[f"{name}_wmax"])
    assert np.any(z["A_count"] == 0) and int((z["A_count"] > 0).sum()) > 400  # taken and never-taken Gaussians
