"""Absolute screen-space gradients (AbsGS; gsr_backward_abs, backward_raw(absgrad=True), means2D.absgrad).

Truth: tests/absgrad_cases.py -- the oracle's backward called once per pixel, absolute values summed in float64 --
read from tests/golden/absgrad.npz (tests/golden/make_golden_absgrad.py); scene A's is regenerated here.  The bar is
GRAD_CLEAN_TOL, the project's bar against the oracle on Gaussians no threshold flip touches: the scenes have no flip
candidate at all (test_scene_preconditions), so it needs no flip term.  The truth's own decomposition error (the
signed sum of the per-pixel calls against the oracle's one full backward) is ~1e-7 and is asserted below 1e-6.
Achieved figures: profiles/parity_absgrad.json.
"""
import ctypes
import functools
import json

import numpy as np
import pytest
import torch

from tests import absgrad_cases as C
from tests import parity
from tests.helpers import load_golden, rel_l2, run_oracle, settings_for
from tests.test_gpu_parity import GRAD_CLEAN_TOL

f32 = np.float32
SELECTIONS = {"default": {}, "seg_k32": dict(seg_k=32), "guard": dict(guard=1),
              "whole_tile": dict(bwd_seg=0, bwd_parts=1), "part_waves4": dict(bwd_seg=0, bwd_parts=4),
              "part_waves2": dict(bwd_seg=0, bwd_parts=2), "union": dict(bwd_seg=0, bwd_parts=1, bwd_union=1)}
# the walks whose batches and pairs are counted from the back of a tile's list (no checkpoint restarts)
ONE_WALK = ("whole_tile", "part_waves4", "part_waves2", "union")
GRAD_NAMES = ("means3D", "means2D", "opacities", "scales", "rotations", "shs")
# the issue's census of the three scenes (CPU oracle)
CENSUS = {"A": dict(instances=778, longest_tile=372, saturated=145, above_half=191, untouched=12, flip_candidates=0),
          "A2": dict(longest_tile=502, saturated=768, flip_candidates=0),
          "B": dict(big_gaussians=6, most_instances=72, flip_candidates=0)}


@functools.lru_cache(maxsize=None)
def _fixture():
    return load_golden("absgrad")


@functools.lru_cache(maxsize=None)
def _scene(name):
    return C.scene(name, _fixture())


@functools.lru_cache(maxsize=None)
def _truth_A():
    return C.truth("A", fixture=_fixture())


# ---------------------------------------------------------------------------------------------- CPU
def test_scene_preconditions():
    """What the scenes must exercise, asserted from the oracle: in particular no threshold-flip candidate."""
    for name in C.SCENES:
        z = _fixture()
        assert C.input_hash(name) == str(z[f"{name}_input_sha256"]), f"{name}: regenerated inputs differ"
        cen = C.census(run_oracle(_scene(name)[0])[3])
        want = json.loads(str(z[f"{name}_census"]))
        parity.record(f"absgrad_scene_{name}", "oracle_census", cen)
        assert cen == {k: want[k] for k in cen}, (name, cen, want)
        for k, v in CENSUS[name].items():
            assert cen[k] == v, (name, k, cen)
        assert cen["flip_candidates"] == 0
        n, W, H = C.SCENES[name][:3]
        assert W % 16 and H % 16  # both image edges are partial tiles
    a, a2, b = (json.loads(str(_fixture()[f"{s}_census"])) for s in ("A", "A2", "B"))
    assert a["longest_tile"] > 64 and a["longest_tile"] > 32 * 8  # segment restarts, many batches
    assert b["big_gaussians"] >= 1 and b["most_instances"] > 64  # the big_reduce path
    assert a["abs_over_signed_norm"] > 2 and b["abs_over_signed_norm"] > 2  # the two norms are far apart


def test_fixture_truth_regenerates():
    a, s, full, _ = _truth_A()
    z = _fixture()
    assert rel_l2(a, z["A_abs"]) <= 1e-6
    assert rel_l2(s, full) <= 1e-6 and float(z["A_signed_residual"]) <= 1e-6
    for name in C.SCENES:
        assert float(z[f"{name}_signed_residual"]) <= 1e-6
        assert z[f"{name}_abs"].shape == (C.SCENES[name][0], 2) and z[f"{name}_abs"].dtype == np.float64


def test_signed_never_exceeds_abs():
    a, s, full, _ = _truth_A()
    assert np.all(np.abs(s) <= a)  # the same float64 terms: |sum| <= sum | |
    z = _fixture()
    for name in C.SCENES:  # the oracle's one full backward (fp32 sums: its own rounding allowed for)
        inp, dc, di = _scene(name)
        g = run_oracle(inp)[3].backward(dc, di)["means2D"][:, :2].astype(np.float64)
        t = z[f"{name}_abs"]
        assert np.all(np.abs(g) <= t * (1 + 1e-5) + 1e-12), name
        assert np.all(t >= 0)
    assert np.all(z["A_ext_abs"] >= 0) and np.all(z["A_noinv_abs"] >= 0)


def test_struct_layout_and_sizes():
    from gaussian_splatting_lightning_amd import _native
    lib = _native.load()
    A = _native.AbsgradExt
    assert (ctypes.sizeof(A), A.struct_size.offset, A.dL_dmeans2D_abs.offset, A.densify_abs.offset) == (24, 0, 8, 16)
    assert A().struct_size == 24
    # the two existing structs and the ABI version are what they were
    assert ctypes.sizeof(_native.CompositeExt) == 48
    assert ctypes.sizeof(_native.BackwardArgs) == 368  # tests/test_alpha_background_host.py BACKWARD_ARGS_BYTES
    assert lib.gsr_abi_version() == 3 == _native.ABI_VERSION
    # the scratch layout: the existing size is unchanged, the abs rows (8 B per instance and per big Gaussian) follow
    up = lambda n: (n + 255) // 256 * 256  # noqa: E731
    for R, nb in ((0, 0), (1000, 10), (123457, 3)):
        base = up(max(R, 1) * 40) + up(max(nb, 1) * 40) + 256
        assert lib.gsr_bwd_scratch_bytes(R, nb) == base
        assert lib.gsr_bwd_scratch_bytes_abs(R, nb) == base + up(max(R, 1) * 8) + up(max(nb, 1) * 8)


def test_struct_size_versioning():
    """A field the caller's struct_size does not cover reads as NULL / 0: seen through which argument check fires
    first (all of them before any device work; P = -1 is the error behind the abs struct's own checks)."""
    from gaussian_splatting_lightning_amd import _native
    lib = _native.load()
    cb = _native.ALLOC_FN(lambda c, w, b: None)

    def err(ab, **kw):
        a = _native.BackwardArgs(P=-1, W=8, H=8, background=1, **kw)
        rc = lib.gsr_backward_abs(ctypes.byref(a), None, None if ab is None else ctypes.byref(ab), cb, None, None)
        assert rc == 1
        return lib.gsr_last_error().decode()

    assert "P must be" in err(None)
    assert "densify_stats" in err(_native.AbsgradExt(dL_dmeans2D_abs=1, densify_abs=1))
    assert "dL_dmeans2D_abs" in err(_native.AbsgradExt(densify_abs=1), densify_stats=1)
    assert "P must be" in err(_native.AbsgradExt(dL_dmeans2D_abs=1, densify_abs=1), densify_stats=1)
    short = _native.AbsgradExt(dL_dmeans2D_abs=1, densify_abs=1)
    short.struct_size = _native.AbsgradExt.densify_abs.offset  # ends before densify_abs: read as 0
    assert "P must be" in err(short)
    short.struct_size = _native.AbsgradExt.densify_abs.offset + 2  # covered in part: not there
    assert "P must be" in err(short)
    shorter = _native.AbsgradExt(dL_dmeans2D_abs=1, densify_abs=1)
    shorter.struct_size = 8  # ends before the pointer: NULL, and densify_abs 0
    assert "P must be" in err(shorter, densify_stats=1)
    # gsr_backward / gsr_backward_ext are the new entry point with NULL
    a = _native.BackwardArgs(P=-1, W=8, H=8, background=1)
    assert lib.gsr_backward(ctypes.byref(a), cb, None, None) == 1 and b"P must be" in lib.gsr_last_error()


def _cpu_state(P=4):
    from gaussian_splatting_lightning_amd.rasterizer import ForwardState
    e = torch.empty(0, dtype=torch.uint8)
    return ForwardState(torch.zeros(P, 3), None, torch.zeros(P, 3), torch.zeros(P, 1), torch.zeros(P, 3),
                        torch.zeros(P, 4), None, torch.zeros(P, dtype=torch.int32), torch.zeros(3), torch.eye(4),
                        torch.eye(4), torch.zeros(3), e, e, e, 0, 0, 0)


def test_python_argument_validation():
    from gaussian_splatting_lightning_amd.rasterizer import backward_chunked, backward_raw
    inp = _scene("A")[0]
    rs = settings_for(inp, torch.device("cpu"))
    st = _cpu_state()
    with pytest.raises(RuntimeError, match="abs_stats=True needs out\\['densify_stats'\\]"):
        backward_raw(st, rs, None, abs_stats=True)
    with pytest.raises(RuntimeError, match="means2D_abs"):
        backward_raw(st, rs, None, out={"means2D_abs": torch.zeros(4, 3)})
    with pytest.raises(RuntimeError, match="means2D_abs"):
        backward_raw(st, rs, None, absgrad=True, out={"means2D_abs": torch.zeros(4, 2, dtype=torch.float64)})
    with pytest.raises(RuntimeError, match="every chunk"):
        backward_chunked(st, rs, None, None, [(0, 2, {"means2D_abs": torch.zeros(2, 2)}), (2, 4, {})])
    with pytest.raises(RuntimeError, match="abs_stats=True needs"):
        backward_chunked(st, rs, None, None, [(0, 4, {"means2D_abs": torch.zeros(4, 2)})], abs_stats=True)


def test_update_xyz_gradient_takes_the_abs_tensor():
    from gaussian_splatting_lightning_amd import densify

    class G:
        xyz_grad_accum = torch.zeros(3)
        xyz_grad_count = torch.zeros(3)

    signed = torch.tensor([[3.0, 4.0, 0.0], [0.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    absg = torch.tensor([[6.0, 8.0, 0.0], [1.0, 0.0, 0.0], [5.0, 12.0, 0.0]])
    vis = torch.tensor([True, False, True])
    g = G()
    densify.update_xyz_gradient(g, signed, vis)
    assert g.xyz_grad_accum.tolist() == [5.0, 0.0, 1.0] and g.xyz_grad_count.tolist() == [1.0, 0.0, 1.0]
    densify.update_xyz_gradient(g, signed, vis, absgrad=absg)
    assert g.xyz_grad_accum.tolist() == [15.0, 0.0, 14.0] and g.xyz_grad_count.tolist() == [2.0, 0.0, 2.0]


# ---------------------------------------------------------------------------------------------- GPU
def _t(a, dev):
    return None if a is None else torch.as_tensor(np.asarray(a, f32), device=dev)


def _forward(inp, dev, bg=None):
    from gaussian_splatting_lightning_amd.rasterizer import forward_raw
    rs = settings_for(inp, dev)
    if bg is not None:
        rs = rs._replace(bg=_t(bg, dev))
    color, radii, invd, st = forward_raw(_t(inp["means3D"], dev), _t(inp["shs"], dev), None, _t(inp["opacities"], dev),
                                         _t(inp["scales"], dev), _t(inp["rotations"], dev), None, rs)
    return rs, st, radii


def _run(inp, dc, di, dev, knobs=None, bg=None, **kw):
    """Forward + backward_raw under the knobs; the gradients stay on the device."""
    from gaussian_splatting_lightning_amd import _native
    from gaussian_splatting_lightning_amd.rasterizer import backward_raw
    with _native.tuned(**(knobs or {})):
        rs, st, radii = _forward(inp, dev, bg)
        g = backward_raw(st, rs, _t(dc, dev), _t(di, dev), **kw)
        torch.cuda.synchronize()
    g["radii"] = radii
    return g


def _same(a, b, keys, zero_sign=True):
    """Bitwise equal.  zero_sign=False: up to the sign of a zero, for the gradients other than the abs output when the
    zero fill is switched (a Gaussian without gradient gets the fill's +0 or the per-Gaussian arithmetic's -0, as
    before this output existed)."""
    for k in keys:
        assert not torch.isnan(a[k]).any() and torch.equal(a[k], b[k]), k
        if zero_sign or k == "means2D_abs":
            assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


PARITY = [(s, sel) for s in ("A", "A2") for sel in SELECTIONS] + [("B", "default"), ("B", "whole_tile")]


@pytest.mark.gpu
@pytest.mark.parametrize("name,selection", PARITY)
def test_parity_against_the_per_pixel_oracle(gpu_device, name, selection):
    inp, dc, di = _scene(name)
    g = _run(inp, dc, di, gpu_device, SELECTIONS[selection], absgrad=True)
    got = g["means2D_abs"].cpu().numpy()
    assert got.shape == (C.SCENES[name][0], 2) and got.dtype == f32
    err = rel_l2(got, _fixture()[f"{name}_abs"])
    parity.record(f"absgrad_{name}_{selection}", "means2D_abs_rel_l2", dict(rel_l2=err, bar=GRAD_CLEAN_TOL))
    print(name, selection, "means2D_abs rel L2", err)
    assert err <= GRAD_CLEAN_TOL, err
    assert torch.all(g["means2D_abs"][g["radii"] == 0] == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("selection", ["default", "whole_tile", "part_waves4"])
def test_parity_without_inverse_depth(gpu_device, selection):
    inp, dc, _ = _scene("A")
    g = _run(inp, dc, None, gpu_device, SELECTIONS[selection], absgrad=True)
    err = rel_l2(g["means2D_abs"].cpu().numpy(), _fixture()["A_noinv_abs"])
    parity.record(f"absgrad_A_noinv_{selection}", "means2D_abs_rel_l2", dict(rel_l2=err, bar=GRAD_CLEAN_TOL))
    print("no inverse depth", selection, "means2D_abs rel L2", err)
    assert err <= GRAD_CLEAN_TOL, err


@pytest.mark.gpu
@pytest.mark.parametrize("selection", list(SELECTIONS))
def test_parity_with_alpha_gradient_and_background_image(gpu_device, selection):
    """The ABS x EXT kernels: the alpha gradient changes every pixel's q.  Truth: absgrad_cases.truth_ext."""
    inp, dc, di = _scene("A")
    da, image = C.ext_inputs()
    g = _run(inp, dc, di, gpu_device, SELECTIONS[selection], bg=image, grad_out_alpha=_t(da, gpu_device), absgrad=True)
    err = rel_l2(g["means2D_abs"].cpu().numpy(), _fixture()["A_ext_abs"])
    parity.record(f"absgrad_A_ext_{selection}", "means2D_abs_rel_l2", dict(rel_l2=err, bar=GRAD_CLEAN_TOL))
    print("alpha gradient + background image", selection, "means2D_abs rel L2", err)
    assert err <= GRAD_CLEAN_TOL, err
    # a constant image gives the vector background's bits
    vec = np.asarray([0.3, 0.6, 0.9], f32)
    const = np.broadcast_to(vec[:, None, None], image.shape).copy()
    a = _run(inp, dc, di, gpu_device, SELECTIONS[selection], bg=vec, absgrad=True)
    b = _run(inp, dc, di, gpu_device, SELECTIONS[selection], bg=const, absgrad=True)
    _same(a, b, ("means2D_abs", "means2D"))


@pytest.mark.gpu
@pytest.mark.parametrize("name,selection", [("A", s) for s in SELECTIONS] + [("B", "default"), ("B", "whole_tile")])
def test_other_gradients_keep_their_bits_and_calls_repeat(gpu_device, name, selection):
    inp, dc, di = _scene(name)
    plain = _run(inp, dc, di, gpu_device, SELECTIONS[selection])
    assert "means2D_abs" not in plain
    a = _run(inp, dc, di, gpu_device, SELECTIONS[selection], absgrad=True)
    b = _run(inp, dc, di, gpu_device, SELECTIONS[selection], absgrad=True)
    _same(plain, a, GRAD_NAMES)
    _same(a, b, GRAD_NAMES + ("means2D_abs",))
    # abs >= |signed| componentwise, up to the rounding of the signed sum (n fp32 additions of terms that sum to at
    # most abs in magnitude: n eps abs bounds it; n <= the Gaussian's pixels, < 2^15 here)
    ab, sg = a["means2D_abs"].double(), a["means2D"][:, :2].double().abs()
    assert torch.all(sg <= ab * (1 + 2 ** 15 * 2.0 ** -24))
    assert torch.all(a["means2D_abs"][a["radii"] == 0] == 0)
    if name == "A":  # (scene B has no culled Gaussian)
        assert (a["radii"] == 0).any()


def _with_inert_front_gaussian(inp, culled):
    """Scene A with its front-most rendered Gaussian X made inert: opacity 1e-6 (alpha < 1/255 on every pixel: skipped
    by forward and backward alike) and scales x 3 (more tiles).  X stays at the head of its tiles' lists, so every
    instance behind it is counted one further from the back than without it; culled=True moves X behind the camera
    instead (index and P unchanged), which flips the pairing, and the lone instance, of all of those tiles."""
    run = run_oracle(inp)[3]
    g = run.geom()
    on = g["tiles_touched"] > 0
    x = int(np.flatnonzero(on)[np.argmin(g["depths"][on])])
    out = dict(inp, opacities=inp["opacities"].copy(), scales=inp["scales"].copy(), means3D=inp["means3D"].copy())
    out["opacities"][x] = 1e-6
    out["scales"][x] *= 3
    if culled:
        ph = np.asarray([0.0, 0.0, -1.0, 1.0]) @ np.linalg.inv(inp["viewmatrix"].astype(np.float64))
        out["means3D"][x] = (ph[:3] / ph[3]).astype(f32)
    return out, x


@pytest.mark.gpu
@pytest.mark.parametrize("selection", ONE_WALK)
def test_bits_do_not_depend_on_the_pairing(gpu_device, selection):
    inp, dc, di = _scene("A")
    with_x, x = _with_inert_front_gaussian(inp, culled=False)
    without, _ = _with_inert_front_gaussian(inp, culled=True)
    a = _run(with_x, dc, di, gpu_device, SELECTIONS[selection], absgrad=True)
    b = _run(without, dc, di, gpu_device, SELECTIONS[selection], absgrad=True)
    assert a["radii"][x] > 0 and b["radii"][x] == 0
    tiles = (int(a["radii"][x]) * 2 // 16) ** 2
    assert tiles >= 1
    keep = torch.ones(len(a["radii"]), dtype=torch.bool, device=gpu_device)
    keep[x] = False
    assert torch.all(a["means2D_abs"][x] == 0)  # X takes no pixel
    for k in GRAD_NAMES + ("means2D_abs",):
        assert torch.equal(a[k][keep].view(torch.int32), b[k][keep].view(torch.int32)), k


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "B"])
def test_unaligned_nan_prefilled_output_and_fast_paths_agree(gpu_device, name):
    """The output 4 B off a 16-B boundary (the zero fill's odd-word path), NaN-prefilled, under bwd_prezero 0 / 1 and
    bwd_live 0 / 1: all bitwise the default call's."""
    inp, dc, di = _scene(name)
    P = C.SCENES[name][0]
    want = _run(inp, dc, di, gpu_device, absgrad=True)
    for prezero in (0, 1):
        for live in (0, 1):
            buf = torch.full((2 * P + 8,), float("nan"), device=gpu_device)
            assert buf.data_ptr() % 16 == 0
            out = {"means2D_abs": buf[1:1 + 2 * P].view(P, 2)}
            assert out["means2D_abs"].data_ptr() % 16 == 4
            got = _run(inp, dc, di, gpu_device, dict(bwd_prezero=prezero, bwd_live=live), absgrad=True, out=out)
            assert got["means2D_abs"].data_ptr() == out["means2D_abs"].data_ptr()
            _same(want, got, GRAD_NAMES + ("means2D_abs",), zero_sign=False)
            assert torch.isnan(buf[0]) and torch.isnan(buf[1 + 2 * P:]).all()  # nothing written around it


@pytest.mark.gpu
def test_split_backward_gives_the_single_call_bits(gpu_device):
    from gaussian_splatting_lightning_amd.rasterizer import backward_chunked
    inp, dc, di = _scene("B")
    P = C.SCENES["B"][0]
    rs, st, _ = _forward(inp, gpu_device)
    stats = torch.zeros(P, 2, device=gpu_device)
    want = _run(inp, dc, di, gpu_device, absgrad=True, abs_stats=True, out={"densify_stats": stats})
    nan = lambda *s: torch.full(s, float("nan"), device=gpu_device)  # noqa: E731
    full = dict(means2D=nan(P, 3), shs=nan(P, 16, 3), means2D_abs=nan(P, 2), densify_stats=nan(P, 2),
                opacities=nan(P, 1))
    bounds = [0, 7, 41, P]
    chunks = [(a, b, {k: v[a:b] for k, v in full.items()}) for a, b in zip(bounds[:-1], bounds[1:])]
    backward_chunked(st, rs, _t(dc, gpu_device), _t(di, gpu_device), chunks, abs_stats=True)
    torch.cuda.synchronize()
    assert torch.equal(full["means2D_abs"].view(torch.int32), want["means2D_abs"].view(torch.int32))
    assert torch.equal(full["means2D"].view(torch.int32), want["means2D"].view(torch.int32))
    assert torch.equal(full["shs"].view(torch.int32), want["shs"].view(torch.int32))
    assert torch.equal(full["densify_stats"].view(torch.int32), stats.view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "B"])
def test_densify_statistics(gpu_device, name):
    inp, dc, di = _scene(name)
    P = C.SCENES[name][0]
    z = lambda: torch.zeros(P, 2, device=gpu_device)  # noqa: E731
    today = z()
    plain = _run(inp, dc, di, gpu_device, out={"densify_stats": today})
    # without abs_stats the statistics are today's, with or without the abs output
    s1 = z()
    g1 = _run(inp, dc, di, gpu_device, absgrad=True, out={"densify_stats": s1})
    assert torch.equal(s1.view(torch.int32), today.view(torch.int32))
    # with it, [:, 0] is sqrt(x x + y y) of the output, every operation rounded once (reproduced in fp32 on the host)
    s2 = z()
    g2 = _run(inp, dc, di, gpu_device, abs_stats=True, out={"densify_stats": s2})
    _same(g1, g2, GRAD_NAMES + ("means2D_abs",))
    _same(plain, g2, GRAD_NAMES)
    # (numpy: fp32 products and sum, the square root in float64 rounded once more to fp32, which is the correctly
    # rounded fp32 root; a vector maths library's float sqrt need not be)
    ab = g2["means2D_abs"].cpu().numpy()
    sq = ab[:, 0] * ab[:, 0] + ab[:, 1] * ab[:, 1]
    assert sq.dtype == f32
    want = torch.from_numpy(np.sqrt(sq.astype(np.float64)).astype(f32))
    assert torch.equal(s2[:, 0].cpu().view(torch.int32), want.view(torch.int32))
    assert torch.equal(s2[:, 1], (g2["radii"] > 0).float()) and torch.equal(s2[:, 1], today[:, 1])
    assert float(s2[:, 0].sum()) > 2 * float(today[:, 0].sum())
    # a second view accumulates
    _run(inp, dc, di, gpu_device, abs_stats=True, accumulate_stats=True, out={"densify_stats": s2})
    assert torch.equal(s2[:, 0].cpu().view(torch.int32), (want + want).view(torch.int32))
    assert torch.equal(s2[:, 1], 2 * today[:, 1])


@pytest.mark.gpu
def test_autograd_sets_means2D_absgrad(gpu_device):
    from gaussian_splatting_lightning_amd import GaussianRasterizer
    inp, dc, di = _scene("A")
    dev = gpu_device
    raw = _run(inp, dc, di, dev, absgrad=True)
    grads = {}
    for flag in (False, True):
        leaves = {k: _t(inp[k], dev).requires_grad_(True) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
        means2D = torch.zeros(len(inp["means3D"]), 3, device=dev, requires_grad=True)
        rast = GaussianRasterizer(settings_for(inp, dev), absgrad=True) if flag else GaussianRasterizer(settings_for(inp, dev))
        color, radii, invd = rast(means3D=leaves["means3D"], means2D=means2D, opacities=leaves["opacities"],
                                  shs=leaves["shs"], scales=leaves["scales"], rotations=leaves["rotations"])
        ((color * _t(dc, dev)).sum() + (invd * _t(di, dev)).sum()).backward()
        grads[flag] = means2D.grad.clone()
        if flag:
            assert means2D.absgrad.shape == (len(inp["means3D"]), 3) and means2D.absgrad.dtype == torch.float32
            assert torch.equal(means2D.absgrad[:, :2].contiguous().view(torch.int32), raw["means2D_abs"].view(torch.int32))
            assert torch.all(means2D.absgrad[:, 2] == 0) and not means2D.absgrad.requires_grad
        else:
            assert not hasattr(means2D, "absgrad")
    assert torch.equal(grads[False].view(torch.int32), grads[True].view(torch.int32))
    assert torch.equal(grads[True].view(torch.int32), raw["means2D"].view(torch.int32))


@pytest.mark.gpu
def test_empty_scenes(gpu_device):
    from gaussian_splatting_lightning_amd.rasterizer import backward_raw, forward_raw
    inp, dc, di = _scene("A")
    dev = gpu_device
    rs = settings_for(inp, dev)
    e = lambda *s: torch.zeros(0, *s, device=dev)  # noqa: E731
    _, radii, _, st = forward_raw(e(3), e(16, 3), None, e(1), e(3), e(4), None, rs)
    g = backward_raw(st, rs, _t(dc, dev), _t(di, dev), absgrad=True)
    stats = e(2)
    g2 = backward_raw(st, rs, _t(dc, dev), _t(di, dev), abs_stats=True, out={"densify_stats": stats})
    torch.cuda.synchronize()
    assert g["means2D_abs"].shape == (0, 2) and g2["means2D_abs"].shape == (0, 2)
    # every Gaussian behind the camera: nothing rendered, zero rows (the output is NaN-prefilled)
    ph = np.asarray([0.0, 0.0, -1.0, 1.0]) @ np.linalg.inv(inp["viewmatrix"].astype(np.float64))
    behind = dict(inp, means3D=(inp["means3D"] * f32(0.01) + (ph[:3] / ph[3]).astype(f32)).astype(f32))
    P = len(inp["means3D"])
    out = {"means2D_abs": torch.full((P, 2), float("nan"), device=dev), "densify_stats": torch.ones(P, 2, device=dev)}
    g = _run(behind, dc, di, dev, abs_stats=True, accumulate_stats=True, out=out)
    assert torch.all(g["radii"] == 0)
    assert torch.all(g["means2D_abs"] == 0) and torch.all(out["densify_stats"] == 1)
