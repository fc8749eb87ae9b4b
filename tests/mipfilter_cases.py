"""Mip-Splatting's 3D smoothing filter restated in torch, and the inputs of its tests.

The yardstick of tests/test_mipfilter.py and tests/test_mipfilter_host.py: the definitions of the sampling rate, the
filter and the filtered activations as they are written down (include/gsrast.h), evaluated in the
dtype asked for on the fp32 inputs.  float64 is the truth; the same code in float32 on the CPU gives the error an fp32
evaluation makes, from which the activation tests form their bars (tests/mcmc_cases.py: bar).  Nothing here is derived
from the HIP kernels: visibility is three comparisons on a matrix product, the gradients come from autograd on the
restated forward.

seen is compared exactly.  That only means something when no decision sits on a threshold, so every scene generator
asserts, in float64, that no (Gaussian, camera) pair lies within CLEARANCE = 1e-4 relative of any of the three
thresholds -- far above fp32 rounding -- and it drops nothing to get there: the random scenes pass whole under their
seed, the 300-camera scene is built to (ring300), and every Gaussian and every camera of each is compared.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from tests.mcmc_cases import ULP4, bar, max_rel, rel_l2  # noqa: F401  (the project's bar convention)

NEAR, MARGIN, VARIANCE = 0.2, 0.15, 0.2
CLEARANCE = 1e-4
EPS32 = 2.0 ** -24  # half an fp32 ulp, relative


# ---- cameras ----
def look_at(eye, target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0)) -> np.ndarray:
    """Row-vector view matrix (p_view = [p, 1] V) of a camera at `eye` whose +z looks at `target`."""
    eye, target, up = (np.asarray(v, dtype=np.float64) for v in (eye, target, up))
    fwd = target - eye
    fwd /= np.linalg.norm(fwd)
    right = np.cross(up, fwd)
    right /= np.linalg.norm(right)
    upv = np.cross(fwd, right)
    V = np.eye(4)
    V[:3, 0], V[:3, 1], V[:3, 2] = right, upv, fwd
    V[3, :3] = -eye @ V[:3, :3]
    return V


def ring_cameras(V: int, radii=(3.0,), tans=((0.6, 0.4),), sizes=((640, 426),), height=0.5, phase=0.1,
                 wobble=0.25) -> dict:
    """V look-at cameras on a ring about the y axis; camera k takes radii[k % len], tans[k % len] and sizes[k % len].
    A dict of stacked tensors, the second form `cameras` may take: viewmatrix (V,4,4) fp32, the rest float64."""
    vm, tx, ty, w, h = [], [], [], [], []
    for k in range(V):
        a = phase + 2.0 * math.pi * k / V
        r = radii[k % len(radii)] * (1.0 + wobble * math.sin(3.0 * a))  # not a circle: depths differ between cameras
        vm.append(look_at((r * math.cos(a), height * math.cos(2.0 * a), r * math.sin(a))))
        t, s = tans[k % len(tans)], sizes[k % len(sizes)]
        tx.append(t[0]); ty.append(t[1]); w.append(s[0]); h.append(s[1])
    f64 = torch.float64
    return dict(viewmatrix=torch.tensor(np.stack(vm), dtype=torch.float32), tanfovx=torch.tensor(tx, dtype=f64),
                tanfovy=torch.tensor(ty, dtype=f64), width=torch.tensor(w, dtype=f64),
                height=torch.tensor(h, dtype=f64))


def identity_camera(tanx=0.5, tany=0.25, width=100, height=50) -> dict:
    f64 = torch.float64
    return dict(viewmatrix=torch.eye(4).reshape(1, 4, 4).clone(), tanfovx=torch.tensor([tanx], dtype=f64),
                tanfovy=torch.tensor([tany], dtype=f64), width=torch.tensor([float(width)], dtype=f64),
                height=torch.tensor([float(height)], dtype=f64))


def cameras_to(cams: dict, device) -> dict:
    return {k: v.to(device) for k, v in cams.items()}


def as_settings(cams: dict):
    """The same cameras as a sequence of GaussianRasterizationSettings, the first form `cameras` may take."""
    from gaussian_splatting_lightning_amd import GaussianRasterizationSettings as S
    z3, e4 = torch.zeros(3), torch.eye(4)
    return [S(int(cams["height"][k]), int(cams["width"][k]), float(cams["tanfovx"][k]), float(cams["tanfovy"][k]), z3,
              1.0, cams["viewmatrix"][k], e4, 0, z3, False, False, False) for k in range(len(cams["tanfovx"]))]


# ---- the float64 restatement of the sampling rate and the filter ----
def view_space(means3D: torch.Tensor, cams: dict, dtype=torch.float64):
    """(x, y, z) (P,V) each: p_view = [p, 1] viewmatrix."""
    p = means3D.to(dtype)
    vm = cams["viewmatrix"].to(dtype)
    pv = torch.einsum("pi,vij->pvj", p, vm[:, :3, :3]) + vm[None, :, 3, :3]
    return pv[..., 0], pv[..., 1], pv[..., 2]


def thresholds(means3D, cams, near=NEAR, margin=MARGIN, dtype=torch.float64):
    """(visible (P,V) bool, z (P,V), clearance (P,V)): clearance is the smallest relative distance of the pair from
    its three thresholds z = near, |x| = limx z, |y| = limy z."""
    x, y, z = view_space(means3D, cams, dtype)
    limx = ((1 + 2 * margin) * cams["tanfovx"].to(dtype))[None]
    limy = ((1 + 2 * margin) * cams["tanfovy"].to(dtype))[None]
    vis = (z > near) & (x.abs() <= limx * z) & (y.abs() <= limy * z)
    clear = torch.minimum((z - near).abs() / abs(near),
                          torch.minimum((x.abs() - limx * z).abs() / (limx * z).abs(),
                                        (y.abs() - limy * z).abs() / (limy * z).abs()))
    return vis, z, clear


def focal(cams, dtype=torch.float64):
    return cams["width"].to(dtype) / (2 * cams["tanfovx"].to(dtype))


def sampling_rate(means3D, cams, near=NEAR, margin=MARGIN, dtype=torch.float64):
    """(rate (P,), zmin (P,), seen (P,) int32) as defined: over the visible cameras, max fx / z, min z, their count."""
    vis, z, _ = thresholds(means3D, cams, near, margin, dtype)
    inf = torch.tensor(float("inf"), dtype=dtype)
    rate = torch.where(vis, focal(cams, dtype)[None] / z, torch.zeros((), dtype=dtype)).max(1).values
    zmin = torch.where(vis, z, inf).min(1).values
    return rate, zmin, vis.sum(1).to(torch.int32)


def rate_bars(means3D, cams, near=NEAR, margin=MARGIN):
    """Per Gaussian, the derived bound on the fp32 kernel's |rate - rate64| and |zmin - zmin64|: z carries at most
    4 * 2^-24 (|x V02| + |y V12| + |z V22| + |V32|) (three fused multiply-adds on fp32 inputs), fx and the division
    2 ulp more; each taken as the maximum over the Gaussian's visible cameras (0 where there is none)."""
    vis, z, _ = thresholds(means3D, cams, near, margin)
    p = means3D.double().abs()
    col = cams["viewmatrix"].double()[:, :, 2].abs()  # (V,4)
    dz = 4 * EPS32 * (p @ col[:, :3].t() + col[None, :, 3])
    r = focal(cams)[None] / z
    zero = torch.zeros((), dtype=torch.float64)
    rate_bar = torch.where(vis, r * (dz / z + 2 * 2.0 ** -23), zero).max(1).values
    zmin_bar = torch.where(vis, dz, zero).max(1).values
    return rate_bar, zmin_bar


def filter_3d(means3D, cams, variance=VARIANCE, mode="per_camera", near=NEAR, margin=MARGIN, dtype=torch.float64):
    """filter_3D (P,1): sqrt(variance) / rate, or sqrt(variance) zmin / max fx; unseen rows take the seen maximum, and
    with nothing seen the filter is 0."""
    rate, zmin, seen = sampling_rate(means3D, cams, near, margin, dtype)
    vis = seen > 0
    sd = math.sqrt(variance)
    f = sd / rate if mode == "per_camera" else sd * zmin / focal(cams, dtype).max()
    if not bool(vis.any()):
        return torch.zeros_like(f)[:, None]
    return torch.where(vis, f, f[vis].max())[:, None]


# ---- scenes ----
def _checked(means3D, cams, populated=False):
    vis, z, clear = thresholds(means3D, cams)
    closest = float(clear.min()) if clear.numel() else float("inf")
    assert closest > CLEARANCE, f"a pair lies {closest:.3g} from a threshold: choose another seed, drop nothing"
    if populated:  # every category the kernel's branches separate
        seen = vis.sum(1)
        x, y, _ = view_space(means3D, cams)
        in_image = (x.abs() <= cams["tanfovx"][None] * z) & (y.abs() <= cams["tanfovy"][None] * z)
        assert int((seen == 0).sum()) > 0 and int((seen == vis.shape[1]).sum()) > 0
        assert int((vis & ~in_image).sum()) > 0, "no pair in the margin band outside the image"
        assert int((z <= NEAR).sum()) > 0, "no pair at or behind the near plane"
    return means3D, cams


def scene(name: str):
    """(means3D (P,3) fp32, cameras dict) of a named scene; every (Gaussian, camera) pair of it is compared."""
    if name == "ring5":       # P = 1000: a partial last block; every visibility category
        rng = np.random.default_rng(1)
        return _checked(torch.tensor(1.5 * rng.normal(size=(1000, 3)), dtype=torch.float32), ring_cameras(5), True)
    if name == "one_camera":  # P = 257: one block and one thread
        rng = np.random.default_rng(2)
        return _checked(torch.tensor(1.5 * rng.normal(size=(257, 3)), dtype=torch.float32), ring_cameras(1))
    if name == "single":      # P = 1, V = 1
        return _checked(torch.tensor([[0.3, -0.2, 0.4]]), ring_cameras(1))
    if name == "ring300":
        return _checked(*ring300())
    if name == "unseen":      # every Gaussian far above every frustum
        rng = np.random.default_rng(3)
        pts = rng.normal(size=(65, 3)) * 0.2 + np.array([0.0, 40.0, 0.0])
        return _checked(torch.tensor(pts, dtype=torch.float32), ring_cameras(3, height=0.0))
    raise KeyError(name)


def ring300():
    """P = 513, V = 300, three camera groups (k % 3) that differ in radius, field of view and image size, so in fx.
    153 900 generic pairs cannot all clear three thresholds by 1e-4 (about one in 10^4 of them does not, whatever the
    seed), so this scene is built to: level cameras on circles of radius 2.5 / 3.0 / 3.6 look at the origin, and the
    Gaussians sit within 0.05 of the y axis at heights drawn from bands that stay 1 % or more away from the three
    values limy_g r_g = 1.30, 1.95, 1.404 at which a group's frustum ends.  A height decides which groups see a row:
    |h| < 1.2 all 300 cameras, 1.34 .. 1.37 two groups, 1.48 .. 1.85 one, 2.05 .. 2.5 none; which camera of a group
    gives the largest fx / z is decided by the row's 0.05 of offset from the axis."""
    rng = np.random.default_rng(4)
    cams = ring_cameras(300, radii=(2.5, 3.0, 3.6), tans=((0.6, 0.4), (0.35, 0.5), (0.8, 0.3)),
                        sizes=((1920, 1280), (401, 573), (640, 240)), height=0.0, wobble=0.0)
    bands = ((0.0, 1.2), (1.34, 1.37), (1.48, 1.85), (2.05, 2.5))
    b = rng.integers(0, len(bands), 513)
    h = np.array([rng.uniform(*bands[j]) for j in b]) * rng.choice([-1.0, 1.0], 513)
    off = rng.uniform(-0.05, 0.05, (513, 2))
    means = torch.tensor(np.stack([off[:, 0], h, off[:, 1]], 1), dtype=torch.float32)
    seen = thresholds(means, cams)[0].sum(1)
    assert sorted(set(seen.tolist())) == [0, 100, 200, 300]
    return means, cams


SCENES = ("ring5", "one_camera", "single", "ring300")


def boundary_points(near=NEAR, margin=MARGIN):
    """(means3D (12,3), cameras, seen (12,)): under an identity view matrix, one point on each side of each threshold,
    1e-3 relative away from it: z = near (1 +- 1e-3); |x| = limx z (1 +- 1e-3) on both signs of x; the same for y."""
    cams = identity_camera()
    limx, limy = (1 + 2 * margin) * 0.5, (1 + 2 * margin) * 0.25
    e, z = 1e-3, 2.0
    pts, seen = [(0.0, 0.0, near * (1 + e)), (0.0, 0.0, near * (1 - e))], [1, 0]
    for sign in (1.0, -1.0):
        for f, s in ((1 - e, 1), (1 + e, 0)):
            pts.append((sign * limx * z * f, 0.0, z)); seen.append(s)
            pts.append((0.0, sign * limy * z * f, z)); seen.append(s)
    pts.append((0.0, 0.0, -1.0)); seen.append(0)
    pts.append((limx * z * (1 - e), limy * z * (1 - e), z)); seen.append(1)
    means = torch.tensor(pts, dtype=torch.float32)
    vis, _, clear = thresholds(means, cams, near, margin)
    assert vis[:, 0].to(torch.int32).tolist() == seen and float(clear.min()) > 0.5 * e
    return means, cams, torch.tensor(seen, dtype=torch.int32)


# ---- the filtered activations ----
def activations(scaling, opacity, rotation, filter_3D, dtype=torch.float64, form="ratio"):
    """(s' (N,3), o' (N,1), unit rotation (N,4)) in `dtype`.  form "ratio": c = prod_k s_k / s'_k, the definition;
    "published": c = sqrt(prod s^2 / prod s'^2), the form of the released code."""
    s = torch.exp(scaling.to(dtype))
    o = torch.sigmoid(opacity.to(dtype)).reshape(-1, 1)
    f = filter_3D.to(dtype).reshape(-1, 1)
    sf = torch.sqrt(s * s + f * f)
    if form == "ratio":
        c = (s / sf).prod(1, keepdim=True)
    else:
        c = torch.sqrt((s * s).prod(1, keepdim=True) / (sf * sf).prod(1, keepdim=True))
    q = rotation.to(dtype)
    return sf, o * c, q / q.norm(dim=1, keepdim=True).clamp_min(1e-12)


def plain_activations(scaling, opacity, rotation, dtype=torch.float64):
    q = rotation.to(dtype)
    return (torch.exp(scaling.to(dtype)), torch.sigmoid(opacity.to(dtype)).reshape(-1, 1),
            q / q.norm(dim=1, keepdim=True).clamp_min(1e-12))


def activation_grads(scaling, opacity, rotation, filter_3D, ups, dtype=torch.float64):
    """dL/d(raw scaling, opacity, rotation) for the upstream gradients `ups` of (s', o', rotations): autograd on the
    restated forward, in `dtype`."""
    leaves = [t.detach().to(dtype).clone().requires_grad_(True) for t in (scaling, opacity.reshape(-1, 1), rotation)]
    out = activations(*leaves, filter_3D, dtype=dtype)
    torch.autograd.backward(out, [u.to(dtype).reshape(o.shape) for u, o in zip(ups, out)])
    return [t.grad for t in leaves]


RANGES = ("ordinary", "f_large", "f_small", "needle", "zero")
SIZES = (1000, 1)


def activation_inputs(case: str, N: int):
    """Raw (scaling (N,3), opacity (N,1), rotation (N,4), filter_3D (N,1)) of one range:
    ordinary  scales 0.005 .. 0.5, f of the same order      f_large  scales 1e-4 .. 1e-3, f 0.1 .. 1
    f_small   scales 0.005 .. 0.5, f 1e-6 .. 1e-5           needle   raw scaling -17 +- 0.5, f = 1e-3
    zero      scales 0.005 .. 0.5, f = 0
    Quaternions are unnormalised with norms from 0.1 to 10."""
    rng = np.random.default_rng(1000 * RANGES.index(case) + N)
    lo, hi = math.log(0.005), math.log(0.5)
    scaling = rng.uniform(lo, hi, (N, 3))
    if case == "ordinary":
        f = np.exp(rng.uniform(lo, hi, (N, 1)))
    elif case == "f_large":
        scaling = rng.uniform(math.log(1e-4), math.log(1e-3), (N, 3))
        f = rng.uniform(0.1, 1.0, (N, 1))
    elif case == "f_small":
        f = np.exp(rng.uniform(math.log(1e-6), math.log(1e-5), (N, 1)))
    elif case == "needle":
        scaling = -17.0 + rng.uniform(-0.5, 0.5, (N, 3))
        scaling[0] = -17.0
        f = np.full((N, 1), 1e-3)
    else:
        f = np.zeros((N, 1))
    o = rng.uniform(0.02, 0.98, (N, 1))
    q = rng.normal(size=(N, 4))
    q *= (10.0 ** rng.uniform(-1, 1, (N, 1))) / np.linalg.norm(q, axis=1, keepdims=True)
    t = lambda a: torch.tensor(a.astype(np.float32))  # noqa: E731
    return t(scaling), t(np.log(o / (1 - o))), t(q), t(f)


def upstream(N: int, seed: int = 7):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(N, w, generator=g) for w in (3, 1, 4)]


_REFERENCE: dict = {}


def activation_reference(case: str, N: int) -> dict:
    """Computed once per (range, size) and shared: the inputs, the upstream gradients, the float64 outputs and
    gradients, and the errors the fp32 CPU restatement of the ratio form makes against them (what the bars are made of).
    Forward errors are maxima of the relative error, gradient errors relative L2 over the tensor."""
    key = (case, N)
    if key not in _REFERENCE:
        inp = activation_inputs(case, N)
        ups = upstream(N)
        out64 = activations(*inp)
        out32 = activations(*inp, dtype=torch.float32)
        g64 = activation_grads(*inp, ups)
        g32 = activation_grads(*inp, ups, dtype=torch.float32)
        fp32 = dict(scales=max_rel(out32[0], out64[0]), opacities=max_rel(out32[1], out64[1]),
                    d_scaling=rel_l2(g32[0], g64[0]), d_opacity=rel_l2(g32[1], g64[1]),
                    d_rotation=rel_l2(g32[2], g64[2]))
        _REFERENCE[key] = dict(inputs=inp, ups=ups, out64=out64, g64=g64, fp32_error=fp32)
    return _REFERENCE[key]
