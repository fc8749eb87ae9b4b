"""Camera gradients, the parts that need no GPU: the C ABI's new fields and version, argument validation before any
device call, and the internal consistency of the reference fixture (tests/golden/camgrad.npz)."""
import ctypes
import os
import re

import numpy as np

from gaussian_splatting_lightning_amd import _native
from tests.camera_cases import BIG_CASE, CAMERA_KEYS, CASES, UNSAT_CASES, load_case, translation_residual
from tests.helpers import load_golden

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gsrast.h")
NEW_FIELDS = ("dL_dviewmatrix", "dL_dprojmatrix", "dL_dcampos")


def test_backward_args_end_with_the_camera_outputs_in_header_order():
    B = _native.BackwardArgs
    names = [n for n, _ in B._fields_]
    assert tuple(names[-3:]) == NEW_FIELDS
    ptr = ctypes.sizeof(ctypes.c_void_p)
    for k, n in enumerate(NEW_FIELDS):  # three pointers closing the struct, nothing behind them
        assert getattr(B, n).offset == ctypes.sizeof(B) - (3 - k) * ptr, n
    # the header declares them last, in the same order
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct gsr_backward_args \{(.*?)\} gsr_backward_args;", txt, flags=re.S).group(1)
    declared = re.findall(r"\*?\s*(\w+)\s*[,;]", body)
    assert tuple(declared[-3:]) == NEW_FIELDS
    assert declared.index("campos_nrows") == len(declared) - 4
    assert re.search(r"GSR_BUF_CAMERA_PARTIALS\s*=\s*4\b", txt) and _native.GSR_BUF_CAMERA_PARTIALS == 4


def test_abi_version_is_3():
    assert _native.load().gsr_abi_version() == _native.ABI_VERSION == 3
    assert re.search(r"#define GSR_ABI_VERSION 3\b", open(HEADER).read())


def test_invalid_backward_arguments_fail_before_touching_the_device():
    """On a host without a GPU a device call would fail with GSR_ERR_HIP (2); these return GSR_ERR_ARG (1), and the
    allocation callback -- the camera partials' included -- is never reached."""
    lib = _native.load()
    asked = []

    def alloc(_ctx, which, nbytes):
        asked.append((which, nbytes))
        return None

    cb = _native.ALLOC_FN(alloc)
    cam = dict(dL_dviewmatrix=1, dL_dprojmatrix=1, dL_dcampos=1)
    ok = dict(P=5, W=10, H=10, D=0, M=1, means3D=1, opacities=1, viewmatrix=1, projmatrix=1, background=1, shs=1,
              campos=1, scales=1, rotations=1, dL_dpix=1, radii=1, geom_buffer=1, image_buffer=1, dL_dsh=1)
    for bad, msg in ((dict(P=-1), b"P must be"), (dict(g_begin=3, g_end=2), b"Gaussian range"),
                     (dict(g_begin=0, g_end=6), b"Gaussian range"), (dict(stages=7), b"backward stages"),
                     (dict(dL_dpix=None), b"dL_dpix"), (dict(geom_buffer=None), b"forward buffers"),
                     (dict(stages=_native.GSR_BWD_GAUSSIANS, R=10, binning_buffer=1), b"bwd_scratch")):
        a = _native.BackwardArgs(**{**ok, **cam, **bad})
        assert lib.gsr_backward(ctypes.byref(a), cb, None, None) == 1, bad
        assert msg in lib.gsr_last_error(), (bad, lib.gsr_last_error())
    assert asked == []


def test_fixture_is_consistent():
    z = load_golden("camgrad")
    assert set(z) == {f"{c}_{k}" for c in CASES for k in CAMERA_KEYS} | {BIG_CASE + "_mask_bits",
                                                                        BIG_CASE + "_input_sha256"}
    for c in CASES:
        inp, dc, di, ref = load_case(c, z)  # (the big case: asserts the regenerated inputs' SHA-256)
        assert ref["viewmatrix"].shape == (4, 4) and ref["projmatrix"].shape == (4, 4) and ref["campos"].shape == (3,)
        assert all(ref[k].dtype == np.float32 and np.isfinite(ref[k]).all() and ref[k].any() for k in CAMERA_KEYS)
        assert not ref["viewmatrix"][:, 3].any() and not ref["projmatrix"][:, 2].any()
        assert dc.shape == (3, inp["image_height"], inp["image_width"])
    W, H = 208, 144
    mask = np.unpackbits(z[BIG_CASE + "_mask_bits"])[:W * H]
    assert 0 < (mask == 0).sum() < 0.01 * W * H  # a few threshold-flip candidate pixels left out, not the image


def test_fixture_satisfies_the_translation_identity():
    """The reference's three camera gradients together with its dL/dmeans3D of the same run (stored in the cases' own
    fixtures): residual <= 1e-6 of the scale, per component."""
    z = load_golden("camgrad")
    for c in UNSAT_CASES:
        inp, _dc, _di, ref = load_case(c, z)
        dm = load_golden(c)["ref_grad_means3D"].astype(np.float64)
        res, scale = translation_residual(inp["viewmatrix"], inp["projmatrix"], dm.sum(0), ref["viewmatrix"],
                                          ref["projmatrix"], ref["campos"], np.abs(dm).sum(0))
        print(c, "residual", res, "scale", scale)
        assert np.all(np.abs(res) <= 1e-6 * scale), (c, res, scale)
