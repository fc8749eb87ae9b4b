"""3DGS-MCMC noise / relocation / growth (csrc/gsr_mcmc.hip), the parts that need no GPU: the three exported symbols and
their declarations, every argument refusal before any device work, the empty calls, the Python validation errors, the
source draw's two routes, and the identities of the float64 restatement the GPU tests are measured against."""
import ctypes
import math
import os
import re
import types

import pytest
import torch

from gaussian_splatting_lightning_amd import _native
from tests import mcmc_cases as MC

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gsrast.h")
GSR_OK, GSR_ERR_ARG = 0, 1
NAMES = ("gsr_mcmc_noise", "gsr_mcmc_relocation", "gsr_mcmc_apply")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_library_exports_the_entry_points():
    lib = _native.load()
    for name in NAMES:
        assert name in _native.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert re.search(r"\bint " + name + r"\(", _header()), name
        assert getattr(lib, name).restype is ctypes.c_int
    assert lib.gsr_abi_version() == _native.ABI_VERSION == 3  # new entry points, not a new ABI


def _c_params(name):
    """The C parameter list of a declaration in the header as 'ptr' / the scalar type."""
    body = re.search(r"\bint " + name + r"\((.*?)\);", _header(), flags=re.S).group(1)
    out = []
    for prm in body.split(","):
        prm = " ".join(prm.split())
        out.append("ptr" if "*" in prm else prm.rsplit(" ", 1)[0].replace("const ", ""))
    return out


def test_ctypes_signatures_match_the_header():
    lib = _native.load()
    kinds = {"ptr": (ctypes.c_void_p,), "int64_t": (ctypes.c_int64,), "int": (ctypes.c_int,), "float": (ctypes.c_float,)}
    for name in NAMES:
        want = _c_params(name)
        got = getattr(lib, name).argtypes
        assert len(got) == len(want), name
        for w, g in zip(want, got):
            assert g in kinds[w] or (w == "ptr" and issubclass(g, ctypes._Pointer)), (name, w, g)
    # the field struct gsr_mcmc_apply shares with gsr_densify_apply, and the kind only it takes
    F = _native.DensifyField
    assert [n for n, _ in F._fields_] == ["src", "dst", "src_exp_avg", "src_exp_avg_sq", "dst_exp_avg",
                                          "dst_exp_avg_sq", "width", "kind"]
    assert ctypes.sizeof(F) == 56 and F.width.offset == 48 and F.kind.offset == 52
    assert re.search(r"GSR_FIELD_OPACITY = (\d+)", _header()).group(1) == str(_native.FIELD_OPACITY) == "4"
    assert re.search(r"GSR_FIELD_STAT = (\d+)", _header()).group(1) == str(_native.FIELD_STAT)


def _fields(**change):
    """The six parameter fields with made-up addresses (never dereferenced by a refused or empty call)."""
    widths = dict(xyz=3, features_dc=3, features_rest=45, opacity=1, scaling=3, rotation=4)
    kinds = dict(opacity=_native.FIELD_OPACITY, scaling=_native.FIELD_SCALING)
    out = []
    for k, w in widths.items():
        f = dict(src=4096, dst=8192, src_exp_avg=None, src_exp_avg_sq=None, dst_exp_avg=None, dst_exp_avg_sq=None,
                 width=w, kind=kinds.get(k, _native.FIELD_PLAIN))
        if change.get(k, {}).get("drop"):
            continue
        f.update(change.get(k, {}))
        out.append(_native.DensifyField(*[f[n] for n, _ in _native.DensifyField._fields_]))
    return (_native.DensifyField * len(out))(*out), len(out)


def _refused(rc, lib, what):
    # on a host without a GPU a device call would give GSR_ERR_HIP (2): GSR_ERR_ARG shows the refusal came first
    assert rc == GSR_ERR_ARG, (what, rc)
    assert b"mcmc" in lib.gsr_last_error(), what


def test_invalid_arguments_fail_before_any_device_work():
    lib = _native.load()
    P = 4096  # a made-up, 16-B aligned address
    # noise: (N, xyz, opacity, scaling, rotation, z, scale, stream)
    ok = [5, P, P, P, P, P, 80.0, None]
    for i in range(1, 6):
        a = list(ok)
        a[i] = None
        _refused(lib.gsr_mcmc_noise(*a), lib, f"noise null {i}")
    _refused(lib.gsr_mcmc_noise(-1, P, P, P, P, P, 80.0, None), lib, "noise N < 0")
    _refused(lib.gsr_mcmc_noise(5, P, P, P, P + 4, P, 80.0, None), lib, "noise misaligned rotation")
    # relocation: (N, opacity, scaling, activated, src_idx, ratio, n, min_opacity, new_opacity, new_scaling, stream)
    ok = [9, P, P, 0, P, P, 5, 0.005, P, P, None]
    for i in (1, 2, 5, 8, 9):
        a = list(ok)
        a[i] = None
        _refused(lib.gsr_mcmc_relocation(*a), lib, f"relocation null {i}")
    for i, bad in ((0, -1), (6, -1), (7, 0.0), (7, 1.0), (7, -0.5), (7, 1.5), (7, float("nan"))):
        a = list(ok)
        a[i] = bad
        _refused(lib.gsr_mcmc_relocation(*a), lib, f"relocation arg {i} = {bad}")
    a = list(ok)
    a[4], a[6] = None, 10  # rows themselves as sources, but more of them than there are rows
    _refused(lib.gsr_mcmc_relocation(*a), lib, "relocation n > N without src_idx")
    # apply: (N, n, src_idx, dst_idx, occurrences, min_opacity, values, fields, num_fields, stream)
    arr, nf = _fields()
    ok = [9, 5, P, P, P, 0.005, P, arr, nf, None]
    for i in (2, 4, 6, 7):
        a = list(ok)
        a[i] = None
        _refused(lib.gsr_mcmc_apply(*a), lib, f"apply null {i}")
    for i, bad in ((0, -1), (1, -1), (5, 0.0), (5, 1.0), (8, -1), (8, 17)):
        a = list(ok)
        a[i] = bad
        _refused(lib.gsr_mcmc_apply(*a), lib, f"apply arg {i} = {bad}")
    for mode in (P, None):  # relocate, add
        for change, what in ((dict(xyz=dict(width=0)), "width 0"), (dict(rotation=dict(dst=None)), "no dst"),
                             (dict(opacity=dict(drop=True)), "no opacity field"),
                             (dict(scaling=dict(drop=True)), "no scaling field"),
                             (dict(opacity=dict(width=2)), "opacity width"), (dict(xyz=dict(kind=9)), "bad kind")):
            arr, nf = _fields(**change)
            _refused(lib.gsr_mcmc_apply(9, 5, P, mode, P, 0.005, P, arr, nf, None), lib, what)
    arr, nf = _fields(xyz=dict(src=None))
    _refused(lib.gsr_mcmc_apply(9, 5, P, None, P, 0.005, P, arr, nf, None), lib, "add without src")
    arr, nf = _fields(xyz=dict(dst_exp_avg=P))
    _refused(lib.gsr_mcmc_apply(9, 5, P, None, P, 0.005, P, arr, nf, None), lib, "add: moment without source")


def test_empty_calls_launch_nothing():
    """n = 0 or N = 0: GSR_OK without a device call (which would be GSR_ERR_HIP here, and a fault at these addresses)."""
    lib = _native.load()
    P = 4096
    assert lib.gsr_mcmc_noise(0, P, P, P, P, P, 80.0, None) == GSR_OK
    assert lib.gsr_mcmc_relocation(9, P, P, 0, P, P, 0, 0.005, P, P, None) == GSR_OK
    assert lib.gsr_mcmc_relocation(0, P, P, 1, None, P, 0, 0.005, P, P, None) == GSR_OK
    arr, nf = _fields()
    for mode in (P, None):
        assert lib.gsr_mcmc_apply(9, 0, P, mode, P, 0.005, P, arr, nf, None) == GSR_OK
        assert lib.gsr_mcmc_apply(0, 0, P, mode, P, 0.005, P, arr, nf, None) == GSR_OK


def _model(N=6, dead=2, **change):
    p, s = MC.scene(N, seed=3, dead=dead, rest=2)
    g = types.SimpleNamespace(spatial_scale=1.0)
    for k in MC.PARAMETER_NAMES:
        setattr(g, f"_{k}", change.get(k, torch.tensor(p[k])))
    for k in MC.STAT_NAMES:
        setattr(g, k, torch.tensor(s[k]))
    return g


def test_python_argument_validation():
    from gaussian_splatting_lightning_amd import densify
    from gaussian_splatting_lightning_amd.gaussian_model import GaussianModel
    for name in ("inject_noise", "relocate_dead", "add_new"):
        assert callable(getattr(GaussianModel, name)) and name in densify.__all__
    calls = (("inject_noise", lambda g: densify.inject_noise(g, 80.0)),
             ("relocate_dead", lambda g: densify.relocate_dead(g)),
             ("add_new", lambda g: densify.add_new(g, 100)))
    for name, call in calls:
        for k, bad in (("xyz", torch.zeros(6, 4)), ("opacity", torch.zeros(6)), ("opacity", torch.zeros(5, 1)),
                       ("scaling", torch.zeros(6, 3, dtype=torch.float64)), ("rotation", torch.zeros(6, 3)),
                       ("rotation", torch.zeros(6, 8)[:, ::2]), ("features_rest", torch.zeros(7, 2, 3))):
            with pytest.raises(RuntimeError, match=f"{name}: _{k}"):
                call(_model(**{k: bad}))
        # everything valid: the device test is the last thing before a launch, and there is no CPU path
        with pytest.raises(RuntimeError, match="GPU"):
            call(_model())
    for bad in (torch.zeros(5, 3), torch.zeros(6, 3, dtype=torch.float64), torch.zeros(3, 6).t(), [[0.0] * 3] * 6):
        with pytest.raises(RuntimeError, match="noise must be"):
            densify.inject_noise(_model(), 80.0, noise=bad)
    for fn in (densify.relocate_dead, lambda g, **kw: densify.add_new(g, 100, **kw)):
        for bad in (0.0, 1.0, -1.0):
            with pytest.raises(RuntimeError, match="min_opacity"):
                fn(_model(), min_opacity=bad)
    # sampled_idx: two dead rows (0 and 1) of six, so two sources, alive rows of [0, 6)
    for bad, what in ((torch.tensor([2, 6]), "out of range"), (torch.tensor([-1, 3]), "out of range"),
                      (torch.tensor([2, 3, 4]), "shape"), (torch.tensor([2.0, 3.0]), "int64"),
                      (torch.tensor([2, 3], dtype=torch.int32), "int64"), (torch.tensor([2, 1]), "dead row"),
                      ([2, 3], "int64 tensor")):
        with pytest.raises(RuntimeError, match=what):
            densify.relocate_dead(_model(), sampled_idx=bad)
    with pytest.raises(RuntimeError, match="GPU"):
        densify.relocate_dead(_model(), sampled_idx=torch.tensor([2, 5]))
    # add_new at N = 6, cap 8: two new rows
    for bad, what in ((torch.tensor([0, 6]), "out of range"), (torch.tensor([-2, 0]), "out of range"),
                      (torch.tensor([1]), "shape")):
        with pytest.raises(RuntimeError, match=what):
            densify.add_new(_model(), 8, growth=2.0, sampled_idx=bad)
    with pytest.raises(RuntimeError, match="GPU"):
        densify.add_new(_model(), 8, growth=2.0, sampled_idx=torch.tensor([0, 0]))
    o, s, r = MC.relocation_inputs("low", 8)
    for args, what in (((o, s[:, :2], r), "required"), ((o[:7], s, r), "required"), ((o, s, r[:3]), "required"),
                       ((o.double(), s, r), "float32"), ((o, s, r.float()), "integer"), ((o, s, r), "GPU")):
        with pytest.raises(RuntimeError, match=what):
            densify.mcmc_relocation(*args)


def test_source_draw_routes():
    """Up to torch.multinomial's 2^24 categories the draw is torch.multinomial's; above, the inverse of the cumulative
    sum: in range, never a zero-probability row, the same for the same seed, frequencies proportional to the weights."""
    from gaussian_splatting_lightning_amd.densify import _draw_sources
    probs = torch.tensor([0.0, 1.0, 0.0, 3.0, 0.0])
    a = _draw_sources(probs, 1000, torch.Generator().manual_seed(1))
    assert torch.equal(a, torch.multinomial(probs, 1000, replacement=True, generator=torch.Generator().manual_seed(1)))
    b = _draw_sources(probs, 4000, torch.Generator().manual_seed(1), multinomial_max=4)
    assert torch.equal(b, _draw_sources(probs, 4000, torch.Generator().manual_seed(1), multinomial_max=4))
    assert b.dtype == torch.int64 and set(b.tolist()) == {1, 3}
    share = float((b == 3).float().mean())  # binomial(4000, 0.75): sigma 0.0068
    assert abs(share - 0.75) < 0.035


def test_restatement_identities():
    """r = 1: o' = o and c = 1 to rounding.  The hockey-stick closed form equals the double loop for r = 1..51."""
    o = torch.tensor([0.005, 0.02, 0.3, 0.5, 0.9, 0.99, 1 - 1e-6], dtype=torch.float32)
    s = torch.ones(len(o), 3)
    new_o, c, new_s = MC.relocation(o, s, torch.ones(len(o), dtype=torch.int32))
    # 1 - (1 - o) is o to half an ulp of one, so c = o / o' is one to that over the smallest o
    assert float((new_o - o.double()).abs().max()) <= 2.0 ** -53
    assert float((c - 1).abs().max()) <= 2.0 ** -52 / float(o.min())
    assert torch.equal(new_s, c[:, None].expand(-1, 3))
    for r in range(1, MC.R_MAX + 1):
        rr = torch.full((len(o),), r, dtype=torch.int32)
        new_o, c, _ = MC.relocation(o, s, rr)
        new_o2, D = MC.relocation_closed_form(o, rr)
        assert torch.equal(new_o, new_o2)
        # both sums cancel from terms of up to 1e4 times the result at r = 51: 1e-10 relative is 1e6 float64 ulp
        assert MC.max_rel(o.double() / D, c) <= 1e-10, r
        # relocation preserves the rendered mass to first order: r copies of opacity o' stand for one of opacity o
        assert bool((new_o <= o.double() * (1 + 1e-15)).all()) and bool((new_o * r >= o.double() * (1 - 1e-10)).all())
    # the clamp: a ratio of 60 is a ratio of 51, one of 0 a ratio of 1
    a = MC.relocation(o, s, torch.full((len(o),), 60, dtype=torch.int32))
    b = MC.relocation(o, s, torch.full((len(o),), 51, dtype=torch.int32))
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    a = MC.relocation(o, s, torch.zeros(len(o), dtype=torch.int32))
    b = MC.relocation(o, s, torch.ones(len(o), dtype=torch.int32))
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    # the coefficients the double loop uses stay exact integers in float64 (C(50, 25) < 2^53)
    assert math.comb(50, 25) < 2 ** 53
    # the noise restatement: the update is Sigma v, symmetric positive definite, so v . update > 0; gate(0.005) = 1/2
    op, sc, q, z = MC.noise_inputs(63)
    upd, gate = MC.noise(op, sc, q, z, 1.0)
    assert bool(((upd * z.double()).sum(1) > 0).all())
    half = MC.noise(torch.log(torch.tensor([[0.005 / 0.995]], dtype=torch.float64)), sc[:1], q[:1], z[:1], 1.0)[1]
    assert abs(float(half) - 0.5) < 1e-9
    assert int((gate >= MC.NOISE_GATE_MIN).sum()) >= 21 and float(gate[1]) < 1e-20
