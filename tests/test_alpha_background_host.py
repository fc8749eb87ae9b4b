"""Rendered alpha, per-pixel background and background gradients, the parts that need no GPU: the side struct
gsr_composite_ext in the header and in ctypes, the two new entry points, the unchanged version-3 ABI, and argument
validation before any device call or allocation."""
import ctypes
import os
import re

from gaussian_splatting_lightning_amd import _native

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gsrast.h")
EXT_FIELDS = ("struct_size", "background_image", "out_alpha", "dL_dalpha", "dL_dbackground", "dL_dbackground_image")
# ctypes.sizeof of the two argument structs on the commit before gsr_composite_ext existed (LP64)
FORWARD_ARGS_BYTES, BACKWARD_ARGS_BYTES = 176, 368


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_composite_ext_matches_the_header():
    E = _native.CompositeExt
    assert tuple(n for n, _ in E._fields_) == EXT_FIELDS
    assert E.struct_size.offset == 0 and E.struct_size.size == ctypes.sizeof(ctypes.c_size_t)
    ptr = ctypes.sizeof(ctypes.c_void_p)
    for k, n in enumerate(EXT_FIELDS[1:]):  # five pointers behind the size, nothing else
        assert getattr(E, n).offset == ctypes.sizeof(ctypes.c_size_t) + k * ptr, n
    assert ctypes.sizeof(E) == ctypes.sizeof(ctypes.c_size_t) + 5 * ptr
    assert E().struct_size == ctypes.sizeof(E)  # the constructor fills the size the caller was built with
    body = re.search(r"typedef struct gsr_composite_ext \{(.*?)\} gsr_composite_ext;", _header(), flags=re.S).group(1)
    assert tuple(re.findall(r"\*?\s*(\w+)\s*;", body)) == EXT_FIELDS
    assert re.search(r"GSR_BUF_BACKGROUND_PARTIALS\s*=\s*5\b", _header()) and _native.GSR_BUF_BACKGROUND_PARTIALS == 5


def test_library_exports_the_ext_entry_points():
    lib = _native.load()
    for name in ("gsr_forward_ext", "gsr_backward_ext"):
        assert name in _native.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert re.search(r"\bint " + name + r"\(", _header()), name


def test_abi_version_and_argument_structs_are_unchanged():
    assert _native.load().gsr_abi_version() == _native.ABI_VERSION == 3
    assert re.search(r"#define GSR_ABI_VERSION 3\b", open(HEADER).read())
    assert ctypes.sizeof(_native.ForwardArgs) == FORWARD_ARGS_BYTES
    assert ctypes.sizeof(_native.BackwardArgs) == BACKWARD_ARGS_BYTES
    assert [n for n, _ in _native.BackwardArgs._fields_][-3:] == ["dL_dviewmatrix", "dL_dprojmatrix", "dL_dcampos"]
    assert [n for n, _ in _native.ForwardArgs._fields_][-1] == "num_big_out"


def test_invalid_ext_arguments_fail_before_touching_the_device():
    """On a host without a GPU a device call would fail with GSR_ERR_HIP (2); these return GSR_ERR_ARG (1), and the
    allocation callback -- the background partials' included -- is never reached."""
    lib = _native.load()
    asked = []

    def alloc(_ctx, which, nbytes):
        asked.append((which, nbytes))
        return None

    cb = _native.ALLOC_FN(alloc)
    scene = dict(P=5, W=10, H=10, D=0, M=1, means3D=1, opacities=1, viewmatrix=1, projmatrix=1, shs=1, campos=1,
                 scales=1, rotations=1, radii=1)
    fwd = dict(out_color=1, **scene)
    bwd = dict(dL_dpix=1, geom_buffer=1, image_buffer=1, dL_dsh=1, **scene)
    num = ctypes.c_int64(0)
    full = dict(out_alpha=1, dL_dalpha=1, dL_dbackground=1, dL_dbackground_image=1)

    def both(args_extra, ext):
        a = _native.ForwardArgs(**fwd, **args_extra)
        b = _native.BackwardArgs(**bwd, **args_extra)
        return (lib.gsr_forward_ext(ctypes.byref(a), ctypes.byref(ext), cb, None, None, ctypes.byref(num)),
                lib.gsr_last_error(),
                lib.gsr_backward_ext(ctypes.byref(b), ctypes.byref(ext), cb, None, None), lib.gsr_last_error())

    # neither background nor background_image
    rf, mf, rb, mb = both({}, _native.CompositeExt(**full))
    assert (rf, rb) == (1, 1) and b"background" in mf and b"background" in mb
    # struct_size ends before the first pointer field (the size word alone, or nothing)
    for size in (0, ctypes.sizeof(ctypes.c_size_t), ctypes.sizeof(ctypes.c_size_t) + ctypes.sizeof(ctypes.c_void_p) - 1):
        ext = _native.CompositeExt(background_image=1, **full)
        ext.struct_size = size
        rf, mf, rb, mb = both(dict(background=1), ext)
        assert (rf, rb) == (1, 1) and b"struct_size" in mf and b"struct_size" in mb, size
    # the background gradients need dL_dpix, also without Gaussians
    b = _native.BackwardArgs(**{**bwd, "P": 0, "dL_dpix": None}, background=1)
    assert lib.gsr_backward_ext(ctypes.byref(b), ctypes.byref(_native.CompositeExt(dL_dbackground=1)), cb, None, None) == 1
    assert b"dL_dpix" in lib.gsr_last_error()
    # the plain entry points' own checks are reached through the ext ones too
    b = _native.BackwardArgs(**{**bwd, "stages": 7}, background=1)
    assert lib.gsr_backward_ext(ctypes.byref(b), ctypes.byref(_native.CompositeExt(**full)), cb, None, None) == 1
    assert b"backward stages" in lib.gsr_last_error()
    assert asked == []
