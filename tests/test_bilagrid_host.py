"""Bilateral grid, everything that needs no GPU: the C entry points are declared, exported and bound with the header's
signatures, the ABI version is unchanged, every argument refusal happens before device work (the pointers here are
made-up addresses that are never dereferenced), the Python wrapper's validation, the identity initialisation, and the
reference of tests/bilagrid_cases.py against itself."""
import ctypes
import os
import re

import pytest
import torch

from gaussian_splatting_lightning_amd import BilateralGrid, _native, slice_image, total_variation_loss
from gaussian_splatting_lightning_amd import bilagrid as BG
from tests import bilagrid_cases as BC

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gsrast.h")
NAMES = ("gsr_bilagrid_workspace_bytes", "gsr_bilagrid_slice_forward", "gsr_bilagrid_slice_backward",
         "gsr_bilagrid_tv_num_partials", "gsr_bilagrid_tv_forward", "gsr_bilagrid_tv_backward")
GSR_OK, GSR_ERR_ARG = 0, 1
PTR = 0x10000  # a made-up device address


def _declarations():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(2): (m.group(1).strip(), [p.strip() for p in m.group(3).split(",")])
            for m in re.finditer(r"(\w[\w \*]*?)\b(gsr_bilagrid_\w+)\s*\(([^)]*)\)\s*;", txt)}


def _ctype(decl: str):
    decl = decl.replace("const ", "").strip()
    if decl.endswith("*"):
        return ctypes.POINTER(ctypes.c_int32) if decl.startswith("int32_t") else ctypes.c_void_p
    return {"int": ctypes.c_int, "size_t": ctypes.c_size_t}[decl]


def test_symbols_declared_exported_and_bound_as_declared():
    decls = _declarations()
    assert set(decls) == set(NAMES)
    lib = _native.load()
    for name, (ret, params) in decls.items():
        assert name in _native.EXPORTED_SYMBOLS
        fn = getattr(lib, name)
        want = []
        for p in params:
            want.append(_ctype(re.match(r"(.*?)\w+$", p).group(1)))  # "const float *grids" -> "const float *"
        assert list(fn.argtypes) == want, name
        assert fn.restype is _ctype(ret), name


def test_abi_version_unchanged():
    assert _native.ABI_VERSION == 3 and _native.load().gsr_abi_version() == 3
    assert re.search(r"#define GSR_ABI_VERSION 3\b", open(HEADER).read())


def _idx(*values):
    return (ctypes.c_int32 * len(values))(*values)


def _forward(lib, num=2, L=8, Gh=16, Gw=16, grids=PTR, B=1, H=8, W=8, image=PTR, idx=None, out=PTR):
    return lib.gsr_bilagrid_slice_forward(num, L, Gh, Gw, grids, B, H, W, image, _idx(0) if idx is None else idx, out,
                                          None)


def _backward(lib, num=2, L=8, Gh=16, Gw=16, grids=PTR, B=1, H=8, W=8, image=PTR, idx=None, dout=PTR, dgrids=PTR,
              dimage=PTR, ws=None):
    return lib.gsr_bilagrid_slice_backward(num, L, Gh, Gw, grids, B, H, W, image, _idx(0) if idx is None else idx,
                                           dout, dgrids, dimage, ws, None)


@pytest.mark.parametrize("call", [_forward, _backward])
def test_slice_refusals_before_device_work(call):
    lib = _native.load()
    for size in ("num", "L", "Gh", "Gw", "B", "H", "W"):
        for bad in (0, -3):
            assert call(lib, **{size: bad}) == GSR_ERR_ARG, (size, bad)
            assert b"positive" in lib.gsr_last_error()
    for ptr in ("grids", "image", "dout" if call is _backward else "out"):
        assert call(lib, **{ptr: None}) == GSR_ERR_ARG, ptr
        assert b"null" in lib.gsr_last_error()
    assert call(lib, idx=ctypes.POINTER(ctypes.c_int32)()) == GSR_ERR_ARG
    for bad in (-1, 2, 2 ** 31 - 1):
        assert call(lib, idx=_idx(bad)) == GSR_ERR_ARG, bad
        assert b"outside [0, num)" in lib.gsr_last_error()
    assert call(lib, B=3, idx=_idx(1, 0, 2)) == GSR_ERR_ARG  # the last of a batch
    assert call(lib, L=2 ** 20, Gh=2 ** 10, Gw=2 ** 10) == GSR_ERR_ARG and b"too large" in lib.gsr_last_error()
    assert call(lib, W=2 ** 30) == GSR_ERR_ARG and b"too large" in lib.gsr_last_error()


def test_backward_empty_call_and_workspace():
    lib = _native.load()
    # nothing asked for: GSR_OK without touching the device (the arguments are still checked)
    assert _backward(lib, dgrids=None, dimage=None) == GSR_OK
    assert _backward(lib, dgrids=None, dimage=None, idx=_idx(5)) == GSR_ERR_ARG
    # a split support needs the workspace the query reports; most shapes need none
    assert lib.gsr_bilagrid_workspace_bytes(8, 16, 16, 1080, 1920) % (4 * 12 * 8 * 16 * 16) == 0
    assert lib.gsr_bilagrid_workspace_bytes(8, 16, 16, 64, 96) == 0
    need = lib.gsr_bilagrid_workspace_bytes(1, 1, 1, 1080, 1920)
    assert need > 0 and need % (4 * 12) == 0
    assert _backward(lib, L=1, Gh=1, Gw=1, H=1080, W=1920, ws=None) == GSR_ERR_ARG
    assert b"workspace" in lib.gsr_last_error()
    assert lib.gsr_bilagrid_workspace_bytes(0, 16, 16, 64, 96) == 0 == lib.gsr_bilagrid_workspace_bytes(8, 16, 16, 0, 9)


def test_tv_refusals_before_device_work():
    lib = _native.load()
    for k in range(4):
        for bad in (0, -1):
            sizes = [2, 8, 16, 16]
            sizes[k] = bad
            assert lib.gsr_bilagrid_tv_forward(*sizes, PTR, PTR, None) == GSR_ERR_ARG
            assert lib.gsr_bilagrid_tv_backward(*sizes, PTR, PTR, PTR, None) == GSR_ERR_ARG
            assert lib.gsr_bilagrid_tv_num_partials(*sizes) == 0
    assert lib.gsr_bilagrid_tv_forward(2, 8, 16, 16, None, PTR, None) == GSR_ERR_ARG
    assert lib.gsr_bilagrid_tv_forward(2, 8, 16, 16, PTR, None, None) == GSR_ERR_ARG
    for args in ((None, PTR, PTR), (PTR, None, PTR), (PTR, PTR, None)):
        assert lib.gsr_bilagrid_tv_backward(2, 8, 16, 16, *args, None) == GSR_ERR_ARG
    assert 1 <= lib.gsr_bilagrid_tv_num_partials(1, 1, 1, 1) <= lib.gsr_bilagrid_tv_num_partials(200, 8, 16, 16) <= 1024


def test_python_validation_names_the_shapes():
    grids, image = BC.identity_grids(2, 8, 16, 16), torch.zeros(3, 5, 7)
    with pytest.raises(RuntimeError, match=r"\(2, 12, 8, 16\)"):
        slice_image(grids[:, :, :, :, 0], image, 0)
    with pytest.raises(RuntimeError, match=r"\(2, 9, 8, 16, 16\)"):
        slice_image(grids[:, :9], image, 0)
    with pytest.raises(RuntimeError, match=r"float64.*\(2, 12, 8, 16, 16\)"):
        slice_image(grids.double(), image, 0)
    with pytest.raises(RuntimeError, match=r"float16"):
        total_variation_loss(grids.half())
    with pytest.raises(RuntimeError, match=r"\(12, 8, 16, 16\)"):
        total_variation_loss(grids[0])
    with pytest.raises(RuntimeError, match=r"\(5, 7\)"):
        slice_image(grids, image[0], 0)
    with pytest.raises(RuntimeError, match=r"\(4, 5, 7\)"):
        slice_image(grids, torch.zeros(4, 5, 7), 0)
    with pytest.raises(RuntimeError, match=r"\(2, 1, 5, 7\)"):
        slice_image(grids, torch.zeros(2, 1, 5, 7), [0, 1])
    with pytest.raises(ValueError, match="3 entries for a batch of 2"):
        slice_image(grids, torch.zeros(2, 3, 5, 7), [0, 1, 0])
    with pytest.raises(ValueError, match="1 entries for a batch of 2"):
        slice_image(grids, torch.zeros(2, 3, 5, 7), torch.tensor([1]))
    with pytest.raises(ValueError, match=r"index 2 outside \[0, 2\)"):
        slice_image(grids, image, 2)
    with pytest.raises(RuntimeError, match="HIP device"):  # valid arguments, but no CPU path
        slice_image(grids, image, 1)
    with pytest.raises(RuntimeError, match="HIP device"):
        total_variation_loss(grids)


def test_identity_initialisation():
    bg = BilateralGrid(3)
    assert bg.grids.shape == (3, 12, 8, 16, 16) and bg.grids.dtype == torch.float32 and bg.grids.requires_grad
    assert torch.equal(bg.grids.detach(), BC.identity_grids(3, 8, 16, 16))
    bg = BilateralGrid(2, grid_X=5, grid_Y=3, grid_W=4)
    assert bg.grids.shape == (2, 12, 4, 3, 5)  # (num, 12, L = grid_W, Gh = grid_Y, Gw = grid_X)
    for c in range(12):
        assert bool((bg.grids[:, c] == (1.0 if c in (0, 5, 10) else 0.0)).all())
    # the identity grid is the identity map under the reference
    image = torch.rand(1, 3, 6, 9, dtype=torch.float64) * 1.4 - 0.2
    out = BC.slice_grid_sample(bg.grids.detach().double(), image, (1,))
    assert float((out - image).abs().max()) <= 1e-14
    with pytest.raises(ValueError):
        BilateralGrid(0)


@pytest.mark.parametrize("case", BC.CASES, ids=lambda c: c.name)
def test_reference_restatements_agree_and_inputs_keep_off_the_kinks(case):
    grids, image, dout = BC.make(case)  # asserts the input condition
    assert BC.input_condition(case, image.double())
    gray = BC.gray_of(image.double())
    if case.H * case.W >= 16 * 16:
        assert bool((gray < 0).any()) and bool((gray > 1).any())  # both clamps are hit
    out, dg, dx = BC.reference(case)  # asserts grid_sample == hat sum, outputs and gradients
    assert out.dtype == torch.float64 and dg.shape == grids.shape and dx.shape == image.shape
    assert bool((dg[~BC.reached_vertices(case)[:, None, None].expand_as(dg)] == 0).all())
    assert all(0 < b < 4e-5 for b in BC.bars(case))  # float32 against float64: a float32-sized figure


def test_input_condition_refuses_a_pixel_on_a_kink():
    case = BC.CASES[0]
    image = BC.make(case)[1].double().clone()
    image[0, :, 3, 4] = 3.0 / (case.L - 1)  # gray = uz / (L - 1) with uz = 3
    assert not BC.input_condition(case, image)
    image[0, :, 3, 4] = 1.0 + 5e-5
    assert not BC.input_condition(case, image)


def test_tv_restatement_on_a_hand_computed_lattice():
    """One 2x2x2 grid, channel 0 = l + 2 j + 4 i, the rest 0: per axis 4 differences in channel 0 of 1, 2 and 4, over
    12 * 1 * 2 * 2 = 48 differences per grid: (4 * 1 + 4 * 4 + 4 * 16) / 48 = 1.75."""
    g = torch.zeros(1, 12, 2, 2, 2, dtype=torch.float64)
    for l in range(2):
        for j in range(2):
            for i in range(2):
                g[0, 0, l, j, i] = l + 2 * j + 4 * i
    assert float(BC.tv_reference(g)) == pytest.approx(1.75, abs=1e-15)
    # divided by num; a size-1 axis contributes nothing
    assert float(BC.tv_reference(torch.cat([g, torch.zeros_like(g)]))) == pytest.approx(0.875, abs=1e-15)
    assert float(BC.tv_reference(g[:, :, :1])) == pytest.approx((4 * 2 + 16 * 2) / 24, abs=1e-15)
    assert float(BC.tv_reference(torch.randn(3, 12, 1, 1, 1, dtype=torch.float64))) == 0.0


def test_module_exports():
    assert BG.__all__ == ["BilateralGrid", "slice_image", "total_variation_loss"]
    import gaussian_splatting_lightning_amd as pkg
    assert pkg.BilateralGrid is BilateralGrid and "slice_image" in pkg.__all__
