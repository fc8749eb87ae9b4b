"""Edge scenes for the clamp and cut-off branches the generator's scenes never reach (tests/test_edge_cases.py on the
CPU, tests/test_edge_parity.py on the GPU, tests/golden/make_golden_edges.py for the reference fixture edges.npz).

Every builder starts from `scene_inputs` (the seeded generator and the "treehill No.0" camera) and edits the arrays on
the CPU; cameras the generator cannot make are built here.  A scene has at most 600 Gaussians and renders at 96x80,
`near_plane` at 208x144.  What each case is for:

  alpha_clamp     o G > 0.99 on many (Gaussian, pixel) pairs: alpha = min(0.99, o G), forward and backward
  aa_floor_all    antialiasing with every Gaussian on the floor max(det_cov / det_cov_plus, 2.5e-5)
  aa_floor_mixed  the same with every second Gaussian above the floor
  near_plane      z_view on both sides of the 0.2 cull, the kept ones with very large footprints (oracle only: A4)
  cam_*           five cameras on one scene: wide, narrow, anamorphic, rolled + pitched, off-centre principal point
  rotations       identity quaternion with equal scales / non-unit quaternions / untouched, SH degree 3
  extremes        o = 0, o = (1/255)(1 +- 1e-3), o = 1, and Gaussians whose tile rectangle is the whole grid

The cases with a reference fixture keep the fixtures' filters: z_view > 0.5 and centres inside
1.29 tan(fov) (the EWA clamp's convention differs outside, Appendix A14).  Their means3D and SH coefficients are the
generator's own draws (filtered, never edited), so the fixture's SHA-256 covers them; every edited array is stored.
"""
from __future__ import annotations

import functools
import hashlib
import math

import numpy as np

from tests.helpers import FLIP_EXCLUDE, REF_STORED_INPUTS, load_golden, scene_inputs, unshuffle_bytes, upstream

W, H = 96, 80
NEAR_W, NEAR_H = 208, 144
PER_GAUSSIAN = ("means3D", "opacities", "scales", "rotations", "shs")
CAMERAS = ("cam_wide", "cam_narrow", "cam_anamorphic", "cam_rolled", "cam_offcentre")
CASES = ("alpha_clamp", "aa_floor_all", "aa_floor_mixed", "near_plane") + CAMERAS + ("rotations", "extremes")
REF_CASES = ("alpha_clamp",) + CAMERAS + ("rotations", "extremes")  # edges.npz: forward + the six gradients
REF_FORWARD_ONLY = ("aa_floor_all",)                                  # edges.npz: the reference's forward alone
ANTIALIASED = ("aa_floor_all", "aa_floor_mixed")
AA_FLOOR = 2.5e-5       # max(det_cov / det_cov_plus, 0.000025)
ALPHA_MAX = 0.99
ALPHA_MIN = 1.0 / 255.0
NEAR = 0.2
BIG_GAUSSIAN_TILES = 64
# Kept pixels of a fixture (the upstream gradients are zero elsewhere).  The CUDA rule stops a pixel when a prefix
# product of (1 - alpha) falls below 1e-4 and the Python rule when one is at or below 1e-4; every prefix product is at
# least the product over ALL of the tile's instances, so a pixel whose full product (float64, from the oracle's
# records) is >= T_KEEP_EDGE = 2e-4 is stopped by neither.  tests/helpers.py T_KEEP = 0.011 would drop every pixel
# with a clamped pair (one alpha = 0.99 leaves T <= 0.01), which is what alpha_clamp is about.
T_KEEP_EDGE = 2e-4
SEED_UPSTREAM = {name: 101 + i for i, name in enumerate(CASES)}
BG = (0.2, 0.5, 0.9)


# ---- float64 restatement of the projection --------------------------------------------------------------------------
def project64(inp: dict) -> dict:
    """The per-Gaussian projection in float64 from the inputs alone: view-space centre, 2D covariance before the +0.3
    dilation, the antialiasing ratio det_cov / det_cov_plus, pixel centre, 3-sigma radius and tile rectangle."""
    f8 = lambda k: np.asarray(inp[k], np.float64)  # noqa: E731
    Wd, Hd = int(inp["image_width"]), int(inp["image_height"])
    m = f8("means3D")
    hom = np.c_[m, np.ones(len(m))]
    t = hom @ f8("viewmatrix")
    ph = hom @ f8("projmatrix")
    ndc = ph[:, :2] / (ph[:, 3:4] + 1e-7)
    pix = np.stack([((ndc[:, 0] + 1.0) * Wd - 1.0) * 0.5, ((ndc[:, 1] + 1.0) * Hd - 1.0) * 0.5], 1)
    z = t[:, 2]
    zs = np.where(np.abs(z) > 1e-12, z, 1e-12)
    tx, ty = float(inp["tanfovx"]), float(inp["tanfovy"])
    fx, fy = Wd / (2.0 * tx), Hd / (2.0 * ty)
    x = np.clip(t[:, 0] / zs, -1.3 * tx, 1.3 * tx) * zs
    y = np.clip(t[:, 1] / zs, -1.3 * ty, 1.3 * ty) * zs
    J = np.zeros((len(m), 2, 3))
    J[:, 0, 0], J[:, 0, 2] = fx / zs, -fx * x / zs ** 2
    J[:, 1, 1], J[:, 1, 2] = fy / zs, -fy * y / zs ** 2
    T = J @ f8("viewmatrix")[:3, :3].T
    q = f8("rotations")
    w, qx, qy, qz = q.T  # as written: the forward does not normalise (Appendix A11)
    R = np.stack([1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - w * qz), 2 * (qx * qz + w * qy),
                  2 * (qx * qy + w * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - w * qx),
                  2 * (qx * qz - w * qy), 2 * (qy * qz + w * qx), 1 - 2 * (qx * qx + qy * qy)], 1).reshape(-1, 3, 3)
    L = R * (f8("scales") * float(inp["scale_modifier"]))[:, None, :]
    cov = T @ (L @ L.transpose(0, 2, 1)) @ T.transpose(0, 2, 1)
    a, b, c = cov[:, 0, 0], cov[:, 0, 1], cov[:, 1, 1]
    det = a * c - b * b
    det_plus = (a + 0.3) * (c + 0.3) - b * b
    mid = 0.5 * (a + c + 0.6)
    lam = mid + np.sqrt(np.maximum(0.1, mid * mid - det_plus))
    radius = np.ceil(3.0 * np.sqrt(lam))
    gx, gy = (Wd + 15) // 16, (Hd + 15) // 16
    rect = np.stack([np.clip(np.trunc((pix[:, 0] - radius) / 16), 0, gx),
                     np.clip(np.trunc((pix[:, 1] - radius) / 16), 0, gy),
                     np.clip(np.trunc((pix[:, 0] + radius + 15) / 16), 0, gx),
                     np.clip(np.trunc((pix[:, 1] + radius + 15) / 16), 0, gy)], 1).astype(np.int64)
    return dict(t=t, z=z, pix=pix, cov=cov, det=det, det_plus=det_plus, ratio=det / det_plus, radius=radius, rect=rect,
                grid=(gx, gy), sigma=np.sqrt(np.maximum(0.5 * (a + c), 0.0)), focal=(fx, fy),
                inside=(np.abs(t[:, 0] / zs) <= 1.29 * tx) & (np.abs(t[:, 1] / zs) <= 1.29 * ty))


def pair_census(run, inp: dict) -> dict:
    """Per pixel, in float64 from the oracle's own records (pixel centre, conic, opacity, sorted instance list, tile
    ranges): the product of (1 - alpha) over ALL of the tile's instances (`T_all`, what the Python rule ends with and
    a lower bound of every prefix the CUDA rule tests), the number of pairs with o G > 0.99 (`clamped`, and
    `clamped_pixels`, one (gaussian, y, x) row per pair), and the position after the last instance of the tile's list
    with alpha >= 1/255 (`last`: the contributor count of a walk that nothing stops)."""
    g = run.geom()
    xy, co = g["xy"].astype(np.float64), g["conic_opacity"].astype(np.float64)
    pl, rg = run.point_list().astype(np.int64), run.ranges().astype(np.int64)
    Wd, Hd = int(inp["image_width"]), int(inp["image_height"])
    gx = (Wd + 15) // 16
    T_all = np.ones((Hd, Wd))
    clamped = np.zeros((Hd, Wd), np.int64)
    last = np.zeros((Hd, Wd), np.int64)
    pairs = []
    for tile, (r0, r1) in enumerate(rg):
        if r1 <= r0:
            continue
        y0, x0 = (tile // gx) * 16, (tile % gx) * 16
        ys, xs = np.mgrid[y0:min(y0 + 16, Hd), x0:min(x0 + 16, Wd)]
        ids = pl[r0:r1]
        dx = xy[ids, 0][:, None, None] - xs[None]
        dy = xy[ids, 1][:, None, None] - ys[None]
        A, B, C, o = (co[ids, k][:, None, None] for k in range(4))
        power = -0.5 * (A * dx * dx + C * dy * dy) - B * dx * dy
        og = o * np.exp(power)
        alpha = np.where((power > 0) | (og < ALPHA_MIN), 0.0, np.minimum(ALPHA_MAX, og))
        hit = (og > ALPHA_MAX) & (power <= 0)
        T_all[ys, xs] = np.prod(1.0 - alpha, 0)
        clamped[ys, xs] = hit.sum(0)
        on = alpha > 0
        last[ys, xs] = np.where(on.any(0), len(ids) - np.argmax(on[::-1], 0), 0)
        k, py, px = np.nonzero(hit)
        pairs.append(np.stack([ids[k], ys[py, px], xs[py, px]], 1))
    pairs = np.concatenate(pairs, 0) if pairs else np.zeros((0, 3), np.int64)
    return dict(T_all=T_all, clamped=clamped, clamped_pixels=pairs, last=last)


def kept_mask(name: str, run, inp: dict, census: dict | None = None) -> np.ndarray:
    """The fixture's pixel mask: stopped by neither termination rule (T_KEEP_EDGE above) and no threshold-flip
    candidate (oracle threshold margin >= FLIP_EXCLUDE, as make_golden_ref.py does).  Pixels with a clamped pair stay
    in alpha_clamp's mask only, whose fixture is made with the pass-through clamp gradient: the unmodified reference,
    which every other fixture is made with, gives a clamped alpha no gradient."""
    census = census or pair_census(run, inp)
    mask = (census["T_all"] >= T_KEEP_EDGE) & (run.threshold_margin() >= FLIP_EXCLUDE)
    return mask if name == "alpha_clamp" else mask & (census["clamped"] == 0)


def flip_touched(run, inp: dict, margin_below: float = FLIP_EXCLUDE) -> np.ndarray:
    """Gaussians some threshold-flip candidate pixel's walk reaches (as compare_forward marks them)."""
    Wd = int(inp["image_width"])
    gx = (Wd + 15) // 16
    pl, rg = run.point_list(), run.ranges().astype(np.int64)
    _, nc = run.image_state()
    touched = np.zeros(run.P, bool)
    ys, xs = np.nonzero(run.threshold_margin() < margin_below)
    for y, x in zip(ys, xs):
        t = (y // 16) * gx + x // 16
        touched[pl[rg[t, 0]: rg[t, 0] + int(nc[y, x])]] = True
    return touched


# ---- cameras ---------------------------------------------------------------------------------------------------------
def set_camera(inp: dict, view, tanfovx: float, tanfovy: float, cx: float = 0.0, cy: float = 0.0) -> dict:
    """Replace the camera of `inp`: row-vector view matrix `view`, projection with 1 / tan(fov) on the diagonal and the
    principal point moved by (cx, cy) in NDC units through the column-vector matrix's [0, 2] and [1, 2] entries
    (znear 0.01, zfar 100 as the generator's)."""
    view = np.asarray(view, np.float64)
    znear, zfar = 0.01, 100.0
    p = np.zeros((4, 4))
    p[0, 0], p[1, 1], p[0, 2], p[1, 2] = 1.0 / tanfovx, 1.0 / tanfovy, cx, cy
    p[3, 2] = 1.0
    p[2, 2], p[2, 3] = (zfar + znear) / (zfar - znear), -(zfar * znear) / (zfar - znear)
    inp["viewmatrix"] = np.ascontiguousarray(view, np.float32)
    inp["projmatrix"] = np.ascontiguousarray(view @ p.T, np.float32)
    inp["campos"] = np.ascontiguousarray(np.linalg.inv(view)[3, :3], np.float32)
    inp["tanfovx"], inp["tanfovy"] = float(tanfovx), float(tanfovy)
    return inp


def _rot(axis: int, deg: float) -> np.ndarray:
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    m = np.eye(4)
    i, j = [(1, 2), (0, 2), (0, 1)][axis]
    m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
    return m


def _keep(inp: dict, keep) -> dict:
    for k in PER_GAUSSIAN:
        inp[k] = np.ascontiguousarray(inp[k][keep])
    return inp


def _reference_filter(inp: dict) -> dict:
    """z_view > 0.5 (Appendix A4) and centres inside 1.29 tan(fov), decided in float64 from the inputs."""
    p = project64(inp)
    return _keep(inp, (p["z"] > 0.5) & p["inside"])


def _isotropic(inp: dict, idx, sigma_px) -> None:
    """Give the Gaussians `idx` three equal scales so that their projected sigma is about `sigma_px` pixels."""
    p = project64(inp)
    s = np.asarray(sigma_px, np.float64) * p["z"][idx] / p["focal"][0]
    inp["scales"][idx] = s[:, None].astype(np.float32)


def _onscreen(p: dict, border: float) -> np.ndarray:
    """Indices of the Gaussians whose centre lies more than `border` pixels inside the 96x80 image."""
    x, y = p["pix"].T
    return np.nonzero((x > border) & (x < W - 1 - border) & (y > border) & (y < H - 1 - border))[0]


def _spread(points: np.ndarray, candidates: np.ndarray, k: int) -> np.ndarray:
    """k of `candidates` (indices into points), far apart: greedy farthest-point selection from the first one."""
    chosen = [int(candidates[0])]
    d = np.linalg.norm(points[candidates] - points[chosen[0]], axis=1)
    while len(chosen) < k:
        j = int(np.argmax(d))
        chosen.append(int(candidates[j]))
        d = np.minimum(d, np.linalg.norm(points[candidates] - points[candidates[j]], axis=1))
    return np.asarray(chosen)


# ---- the cases -------------------------------------------------------------------------------------------------------
ALPHA_CLAMP_OPAQUE = 40
ALPHA_CLAMP_SIGMA = 14.0


def _alpha_clamp(seed=63) -> dict:
    """40 well-separated on-screen Gaussians get o = 0.99 + d, d over [0, 0.01] (denser towards 0.01; the first exactly
    1.0f, the last exactly 0.99) and an isotropic footprint of sigma = 14 d / 0.01 pixels (at least 2).  The area where
    o G > 0.99 is 2 pi sigma^2 d / 0.99 pixels while the area the Gaussian darkens grows with sigma^2 alone, so the
    footprint goes to the Gaussians that clamp: about 2 pi A d / r^2 = 200-250 clamped pairs is what a 96x80 image
    holds on pixels no second near-opaque Gaussian takes below T_KEEP_EDGE (A the image area, r ~ 1.4 the spacing in
    sigmas); sizes and seed were scanned for the census of tests/test_edge_cases.py, from the oracle alone."""
    inp = _reference_filter(scene_inputs(600, W, H, sh_degree=1, seed=seed, opacity_scale=0.02, bg=BG))
    p = project64(inp)
    # the earliest picks are the farthest apart: they get the largest footprints
    idx = _spread(p["pix"], _onscreen(p, 4), ALPHA_CLAMP_OPAQUE)
    u = np.linspace(1.0, 0.0, ALPHA_CLAMP_OPAQUE)
    delta = 0.01 * (1.0 - (1.0 - u) ** 2)
    _isotropic(inp, idx, np.maximum(2.0, ALPHA_CLAMP_SIGMA * delta / 0.01))
    inp["opacities"][idx, 0] = (0.99 + delta).astype(np.float32)
    assert inp["opacities"][idx[0], 0] == np.float32(1.0)
    inp["opaque_idx"] = idx
    return inp


def _aa_floor(mixed: bool) -> dict:
    inp = _reference_filter(scene_inputs(600, W, H, sh_degree=1, seed=62, bg=BG))
    n = len(inp["means3D"])
    rng = np.random.default_rng(62)
    floor = np.ones(n, bool)
    if mixed:
        floor[1::2] = False
    inp["scales"][floor] *= np.float32(3e-4)
    inp["opacities"][:, 0] = rng.uniform(0.8, 0.999, n).astype(np.float32)
    inp["floor_idx"] = np.nonzero(floor)[0]
    return inp


def _near_plane() -> dict:
    inp = scene_inputs(400, NEAR_W, NEAR_H, sh_degree=1, seed=63, opacity_scale=0.05, bg=BG)
    n = len(inp["means3D"])
    rng = np.random.default_rng(63)
    V = inp["viewmatrix"].astype(np.float64)
    z = np.where(np.arange(n) % 2 == 0, rng.uniform(0.12, 0.19, n), rng.uniform(0.21, 0.35, n))
    tx, ty = inp["tanfovx"], inp["tanfovy"]
    pv = np.stack([rng.uniform(-1.1, 1.1, n) * tx * z, rng.uniform(-1.1, 1.1, n) * ty * z, z], 1)
    inp["means3D"] = np.ascontiguousarray((pv - V[3, :3]) @ np.linalg.inv(V[:3, :3]), np.float32)
    # a footprint of a few pixels at these depths, every 20th one x40 (more than BIG_GAUSSIAN_TILES tiles)
    inp["scales"] *= np.float32(0.02)
    inp["scales"][::20] *= np.float32(40.0)   # behind the plane (culled)
    inp["scales"][1::20] *= np.float32(40.0)  # in front of it (kept)
    return inp


def _camera_scene(seed=75) -> dict:
    return scene_inputs(300, W, H, sh_degree=1, seed=seed, opacity_scale=0.05, bg=BG)


def _camera(name: str, seed=75) -> dict:
    inp = _camera_scene(seed)
    V0 = inp["viewmatrix"].astype(np.float64)
    back = lambda d: V0 + np.r_[np.zeros((3, 4)), [[0.0, 0.0, d, 0.0]]]  # noqa: E731  the camera moved back by d
    if name == "cam_wide":
        set_camera(inp, back(-1.5), 1.5, 1.5 * H / W)
    elif name == "cam_narrow":  # from far enough that the scene fills the narrow frustum
        set_camera(inp, back(26.0), 0.08, 0.08 * H / W)
    elif name == "cam_anamorphic":
        set_camera(inp, V0, 0.6, 1.4 * 0.6 * H / W)
    elif name == "cam_rolled":  # rolled 37 degrees about the view axis, then pitched 12 degrees
        set_camera(inp, V0 @ _rot(2, 37.0) @ _rot(0, 12.0), 0.6, 0.6 * H / W)
    elif name == "cam_offcentre":  # principal point off-centre by (0.2 W, -0.15 H) pixels = (0.4, -0.3) in NDC
        set_camera(inp, V0, 0.6, 0.6 * H / W, cx=0.4, cy=-0.3)
    else:
        raise KeyError(name)
    return _reference_filter(inp)


def _rotations(seed=68) -> dict:
    inp = _reference_filter(scene_inputs(300, W, H, sh_degree=3, seed=seed, opacity_scale=0.05, bg=BG))
    n = len(inp["means3D"])
    rng = np.random.default_rng(seed)
    kind = np.arange(n) % 3
    ident = kind == 0  # what create_from_points makes: identity quaternion, three equal scales
    inp["rotations"][ident] = np.array([1.0, 0.0, 0.0, 0.0], np.float32)
    mean = np.exp(np.log(inp["scales"][ident].astype(np.float64)).mean(1, keepdims=True))
    inp["scales"][ident] = mean.astype(np.float32)
    scaled = kind == 1  # non-unit quaternions (Appendix A11): R scales by f^2, the footprint by f^2
    inp["rotations"][scaled] *= rng.uniform(0.5, 2.0, (int(scaled.sum()), 1)).astype(np.float32)
    inp["kind"] = kind
    return inp


def _extremes(seed=72) -> dict:
    """Of the first 200 on-screen Gaussians: 40 with o = 0, 40 just below and 40 just above 1/255, 6 (far apart) with
    o = 1, 4 scaled x50.  inp["class"] names them 0..4 (-1: untouched)."""
    inp =_reference_filter(scene_inputs(400, W, H, sh_degree=1, seed=seed, opacity_scale=0.02, bg=BG))
    n = len(inp["means3D"])
    p = project64(inp)
    onscreen = _onscreen(p, 2)
    cls = np.full(n, -1)
    cls[onscreen[:200]] = np.arange(200) % 5
    third = np.float32(1.0) / np.float32(255.0)
    inp["opacities"][cls == 0] = np.float32(0.0)
    inp["opacities"][cls == 1] = np.float32(float(third) * (1.0 - 1e-3))
    inp["opacities"][cls == 2] = np.float32(float(third) * (1.0 + 1e-3))
    one = _spread(p["pix"], np.nonzero(cls == 3)[0], 6)  # few and far apart: most pixels keep T above T_KEEP_EDGE
    inp["opacities"][one] = np.float32(1.0)
    cls[(cls == 3)] = -1
    cls[one] = 3
    big = np.nonzero(cls == 4)[0][:4]  # x50: the tile rectangle is clamped on all four sides of the grid
    inp["scales"][big] *= np.float32(50.0)
    cls[cls == 4] = -1
    cls[big] = 4
    inp["class"] = cls
    return inp


_BUILDERS = {"alpha_clamp": _alpha_clamp, "aa_floor_all": lambda: _aa_floor(False),
             "aa_floor_mixed": lambda: _aa_floor(True), "near_plane": _near_plane, "rotations": _rotations,
             "extremes": _extremes, **{c: functools.partial(_camera, c) for c in CAMERAS}}
EXTRA_KEYS = ("opaque_idx", "floor_idx", "kind", "class")


@functools.lru_cache(maxsize=None)
def _built(name: str):
    inp = _BUILDERS[name]()
    dc, di = upstream(int(inp["image_width"]), int(inp["image_height"]), SEED_UPSTREAM[name])
    return inp, dc, di


def build(name: str):
    """(inputs, dL_dcolor, dL_dinvdepth) of one case, before any fixture mask (copies: the caller may edit them)."""
    inp, dc, di = _built(name)
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in inp.items()}, dc.copy(), di.copy()


def antialiased(name: str) -> bool:
    return name in ANTIALIASED


def rasterizer_inputs(inp: dict) -> dict:
    return {k: v for k, v in inp.items() if k not in EXTRA_KEYS}


def input_sha256(inp, dc, di) -> str:
    h = hashlib.sha256()
    for a in (inp["means3D"], inp["shs"], dc, di):
        h.update(np.ascontiguousarray(a, np.float32).tobytes())
    return h.hexdigest()


# ---- the fixture -----------------------------------------------------------------------------------------------------
GRAD_KEYS = ("means3D", "means2D", "opacities", "scales", "rotations", "shs")
REF_GAP_FREE = 2.5e-5  # a reference float32-vs-float64 gap above this widens that entry's bar by 2 x gap


@functools.lru_cache(maxsize=None)
def fixture() -> dict:
    return load_golden("edges")


@functools.lru_cache(maxsize=None)
def load_case(name: str) -> dict:
    """One fixture case in the form tests/helpers.py compare_to_reference reads: regenerated inputs (SHA-256 checked,
    the stored ones taken from the fixture), the reference outputs, the kept-pixel mask, the masked upstream gradients
    and, per gradient, the reference's float32-vs-float64 gap."""
    z = fixture()
    inp, dc, di = build(name)
    h = input_sha256(inp, dc, di)
    assert h == str(z[name + "/input_sha256"]), f"{name}: regenerated inputs differ from the generator's ({h})"
    get = lambda k: unshuffle_bytes(z[f"{name}/{k}"], z[f"{name}/shape_{k}"])  # noqa: E731
    for k in REF_STORED_INPUTS:
        inp[k] = get("input_" + k)
    Wd, Hd = inp["image_width"], inp["image_height"]
    mask = np.unpackbits(z[name + "/mask_bits"])[:Wd * Hd].reshape(Hd, Wd).astype(bool)
    out = dict(inp=inp, mask=mask, ref_color=get("ref_color"), ref_invdepth=get("ref_invdepth"),
               ref_radii=z[name + "/ref_radii"])
    if name in REF_CASES:
        m = mask.astype(np.float32)
        out.update(dL_dcolor=dc * m, dL_dinvdepth=di * m, grad_idx=np.arange(len(inp["means3D"])),
                   gap={k: float(z[f"{name}/gap_{k}"]) for k in GRAD_KEYS})
        for k in GRAD_KEYS:
            out["ref_grad_" + k] = get("ref_grad_" + k)
        if name == "alpha_clamp":  # the unmodified reference (zero gradient through a clamped alpha), on record
            rows = z[name + "/plain_rows"]  # the fixture stores the rows that differ
            for k in GRAD_KEYS:
                out["plain_grad_" + k] = out["ref_grad_" + k].copy()
                out["plain_grad_" + k][rows] = get("plain_grad_" + k)
    return out


def reference_bars(z: dict) -> dict:
    """Per-gradient bar against the fixture: REF_GRAD_TOL, plus twice the reference's own float32-vs-float64 gap where
    that gap exceeds REF_GAP_FREE."""
    from tests.helpers import REF_GRAD_TOL
    return {k: REF_GRAD_TOL + (2.0 * g if g > REF_GAP_FREE else 0.0) for k, g in z["gap"].items()}


DIRECT_TOL = 1e-5  # colour / inverse depth on the kept pixels: the bar of test_golden_unsaturated_direct


def compare_with_fixture(z: dict, color, invdepth, radii, final_T, rgb_max, margin, grads=None, record=None) -> dict:
    """One rasterizer's outputs (the HIP path or the oracle) against a case of edges.npz, with the project's existing
    reference bars: compare_to_reference's (radii exact on the rendered Gaussians; colour and inverse depth within
    REF_COLOR_TOL relative L2 and REF_PIXEL_TOL per pixel on the kept pixels; stopped pixels within their
    transmittance bound; flip candidates within REF_FLIP_TOL), test_golden_unsaturated_direct's (every kept pixel
    within 1e-5 in colour and inverse depth) and, per gradient, REF_GRAD_TOL relative L2 over all Gaussians (plus
    twice the reference's own float32-vs-float64 gap where the fixture records one above REF_GAP_FREE)."""
    from tests.helpers import compare_to_reference, rel_l2
    rec = compare_to_reference(z, color, invdepth, radii, final_T, rgb_max, margin, None, record=record)
    m = z["mask"]
    rec["invdepth_maxabs_mask"] = float(np.abs(np.asarray(invdepth)[0] - z["ref_invdepth"][0])[m].max(initial=0))
    if grads is not None:
        bars = reference_bars(z)
        for k in GRAD_KEYS:
            rec["grad_" + k] = rel_l2(np.asarray(grads[k]).reshape(z["ref_grad_" + k].shape), z["ref_grad_" + k])
            rec["bar_" + k] = bars[k]
    if record is not None:
        record(rec)
    assert rec["color_maxabs_mask"] <= DIRECT_TOL and rec["invdepth_maxabs_mask"] <= DIRECT_TOL, rec
    if grads is not None:
        for k in GRAD_KEYS:
            assert rec["grad_" + k] <= rec["bar_" + k], (k, rec)
    return rec


AA_FLOOR_H = np.sqrt(np.float32(AA_FLOOR))  # sqrtf(2.5e-5f): the opacity factor of a Gaussian on the floor


def floor_equivalent(inp: dict) -> dict:
    """The scene whose non-antialiased render equals aa_floor_all's antialiased one: opacities o sqrtf(2.5e-5f),
    the product formed in float32 as the rasterizer forms it."""
    out = dict(inp)
    out["opacities"] = (np.asarray(inp["opacities"], np.float32) * AA_FLOOR_H).astype(np.float32)
    return out
