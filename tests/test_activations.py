"""Parameter activations (activations.py, csrc/gsr_adam.hip) against torch autograd in fp32.

The reference activates its raw parameters in torch (gs_lightning/modules/gaussian_model.py: get_scaling = exp,
get_opacity = sigmoid, get_rotation = torch.nn.functional.normalize) and differentiates them with autograd; the
fused kernels must agree with that to fp32 rounding (tolerance written per check below).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _raw(N, seed, dev):
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(N, 3, generator=g) * 2.0 - 4.0
    o = torch.randn(N, 1, generator=g) * 3.0
    q = torch.randn(N, 4, generator=g)
    q[:5] = 0.0  # clamped norm: normalize divides by eps
    q[5:9] *= 1e-13
    return s.to(dev), o.to(dev), q.to(dev)


@pytest.mark.parametrize("N", [1, 255, 100_003])
def test_activations_match_torch_autograd(N):
    from gaussian_splatting_lightning_amd.activations import GaussianActivations
    dev = torch.device("cuda:0")
    s, o, q = _raw(N, N, dev)
    leaves = [t.clone().requires_grad_(True) for t in (s, o, q)]
    ref = (torch.exp(leaves[0]), torch.sigmoid(leaves[1]), torch.nn.functional.normalize(leaves[2]))
    ours_in = [t.clone().requires_grad_(True) for t in (s, o, q)]
    ours = GaussianActivations.apply(*ours_in)
    g = torch.Generator().manual_seed(7)
    ups = [torch.randn(t.shape, generator=g).to(dev) for t in ref]
    torch.autograd.backward(ref, ups)
    torch.autograd.backward(ours, ups)
    for a, b, name in zip(ours, ref, ("scales", "opacities", "rotations")):
        torch.testing.assert_close(a, b, rtol=2e-6, atol=0.0, msg=name)          # a few fp32 ulps
    for a, b, name in zip(ours_in, leaves, ("d_scaling", "d_opacity", "d_rotation")):
        # the eps-clamped quaternions take gradients ~1e12: relative tolerance only
        torch.testing.assert_close(a.grad, b.grad, rtol=1e-5, atol=1e-6, msg=name)


# ------------------------------------------------------------------------- float64 parity at the edges
#
# The float64 reference below restates exp, sigmoid, normalize(eps = 1e-12) and their chain rule, with the clamp
# branch as the kernel documents it (|q| > eps: d = (g - u (u . g)) / |q|; else q / eps is linear in q: d = g / eps).
# Bounds, derived (ULP = 2^-23):
#   forward   exp and sigmoid: 4 ULP of the value, plus one subnormal quantum 2^-149 where the value is subnormal
#             (sigmoid(-88), sigmoid(-90)); rotations: 4 ULP of the unit quaternion's largest component.
#   backward  d_scaling = g s and d_opacity = g (1 - o) o read the forward's OUTPUT: the float64 derivative is
#             evaluated over the interval the forward bound allows for that output, and 4 ULP of the result are added
#             (plus a quantum where it is subnormal).  At o within an ulp of 1 (x >= 16.6) that interval holds o = 1,
#             where (1 - o) o = 0: the bound is as wide as the derivative itself there, and says so.
#             d_rotation: g - u (u . g) cancels when g is parallel to u: 8 ULP |g| / |q| per component; in the clamp
#             branch one division: 4 ULP of the component.
# Rows whose |q| is within 1e-3 of eps may take either branch; the inputs hold exactly two, one on each side.

ULP = 2.0 ** -23
QUANTUM = 2.0 ** -149
MIN_NORMAL = 2.0 ** -126
NORM_EPS = 1e-12
OPACITY_EDGES = (0.0, 1e-8, -1e-8, 5.0, -5.0, 16.6, -16.6, 17.0, -17.0, 30.0, -30.0, 88.0, -88.0, 90.0, -90.0)
QUAT_NORMS = (0.0, 1e-20, 1e-13, 1e-6, 1.0, 1e3)
THRESHOLD_NORMS = (0.999e-12, 1.001e-12)  # rows 3 and 4
# "within 1e-3 of eps", with room for the fp32 rounding of the two constructed quaternions (2^-24 of their norm)
NEAR = 1e-3 + 2.0 ** -23


def _edge_inputs(N, seed):
    """fp32 (scaling, opacity, rotation, d_scales, d_opacities, d_rotations) as numpy arrays."""
    rng = np.random.default_rng(seed)
    i = np.arange(N)
    o = np.where(i % 16 < 15, np.asarray(OPACITY_EDGES + (0.0,))[i % 16], rng.normal(0.0, 3.0, N))
    s = rng.uniform(-30.0, 10.0, (N, 3))
    s[0, 0], s[-1, -1] = -30.0, 10.0
    d = rng.standard_normal((N, 4))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    axis = i % 5 == 0                      # axis-aligned quaternions, both signs
    d[axis] = 0.0
    d[axis, (i[axis] // 5) % 4] = np.where((i[axis] // 20) % 2 == 0, 1.0, -1.0)
    norms = np.asarray(QUAT_NORMS)[i % len(QUAT_NORMS)]
    if N > 4:
        norms[3:5] = THRESHOLD_NORMS
    q = d * norms[:, None]
    gs, go, gq = rng.standard_normal((N, 3)), rng.standard_normal((N, 1)), rng.standard_normal((N, 4))
    hot = i % 3 == 0                       # upstream gradient 1 in a single component: a swapped component shows
    gs[hot], go[hot], gq[hot] = 0.0, 1.0, 0.0
    gs[hot, (i[hot] // 3) % 3] = 1.0
    gq[hot, (i[hot] // 3) % 4] = 1.0
    return [a.astype(np.float32) for a in (s, o.reshape(N, 1), q, gs, go, gq)]


def _sigmoid_backward64(go, o):
    return go * (1.0 - o) * o


def _reference64(s, o, q, gs, go, gq):
    """Float64 forward values, backward values and their bounds; "near": rows that may take either normalize branch,
    with both branches' (value, bound)."""
    s, o, q, gs, go, gq = (a.astype(np.float64) for a in (s, o, q, gs, go, gq))

    def sub(y):
        return np.where(np.abs(y) < MIN_NORMAL, QUANTUM, 0.0)

    scales = np.exp(s)
    opac = 1.0 / (1.0 + np.exp(-o))
    n = np.sqrt((q * q).sum(axis=1, keepdims=True))
    rot = q / np.maximum(n, NORM_EPS)
    fwd = {"scales": (scales, 4 * ULP * scales + sub(scales)), "opacities": (opac, 4 * ULP * opac + sub(opac)),
           "rotations": (rot, np.broadcast_to(4 * ULP * np.abs(rot).max(axis=1, keepdims=True), rot.shape))}
    # d_scaling = g s over s +- its forward bound
    d_s = gs * scales
    tol_s = np.abs(gs) * fwd["scales"][1] + 4 * ULP * np.abs(d_s) + sub(d_s)
    # d_opacity = g (1 - o) o over o +- its forward bound: a parabola in o, extreme at the ends or at o = 1/2
    d_o = go / (1.0 + np.exp(-o)) / (1.0 + np.exp(o))  # (1 - o) o without the cancellation of 1 - o
    lo, hi = opac - fwd["opacities"][1], opac + fwd["opacities"][1]
    at = _sigmoid_backward64(go, opac)
    span = np.zeros_like(at)
    for pt in (lo, hi, np.clip(0.5, lo, hi)):
        span = np.maximum(span, np.abs(_sigmoid_backward64(go, pt) - at))
    tol_o = span + 4 * ULP * np.abs(d_o) + sub(d_o)
    # d_rotation, both branches
    gnorm = np.sqrt((gq * gq).sum(axis=1, keepdims=True))
    with np.errstate(divide="ignore", invalid="ignore"):
        u = q / n
        full = (gq - u * (u * gq).sum(axis=1, keepdims=True)) / n
        tol_full = np.broadcast_to(8 * ULP * gnorm / n, gq.shape)
    clamp = gq / NORM_EPS
    tol_clamp = 4 * ULP * np.abs(clamp)
    normalized = n > NORM_EPS
    near = (np.abs(n / NORM_EPS - 1.0) <= NEAR).ravel()
    bwd = {"d_scaling": (d_s, tol_s), "d_opacity": (d_o, tol_o),
           "d_rotation": (np.where(normalized, full, clamp), np.where(normalized, tol_full, tol_clamp))}
    return fwd, bwd, {"rows": near, "normalized": normalized.ravel(), "full": (full, tol_full),
                      "clamp": (clamp, tol_clamp)}


def _assert_within(name, got, ref, tol, skip_rows=None):
    got = got.astype(np.float64).reshape(ref.shape)
    assert np.isfinite(got).all(), f"{name}: not finite"
    over = np.abs(got - ref) > tol
    if skip_rows is not None:
        over[skip_rows] = False
    if over.any():
        r, c = np.argwhere(over)[0]
        raise AssertionError(f"{name}: {int(over.sum())} elements out of bound, first at row {r} component {c}: "
                             f"got {got[r, c]!r}, float64 {ref[r, c]!r}, bound {tol[r, c]:.3e}")
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(np.abs(got - ref) == 0, 0.0, np.abs(got - ref) / tol)
    if skip_rows is not None:
        ratio[skip_rows] = 0.0
    return float(ratio.max(initial=0.0))


@pytest.mark.parametrize("N", [1, 255, 256, 257, 1025])
def test_activations_match_float64_at_the_edges(N):
    """One Gaussian, one block less one, exactly one, one more, and five blocks: sigmoid from 0 through saturation
    (|x| = 16.6, 17, 30) to where expf over- and underflows (88, 90), exp over [-30, 10], quaternion norms 0 ... 1e3
    with one row on each side of the 1e-12 clamp."""
    from gaussian_splatting_lightning_amd.activations import GaussianActivations
    dev = torch.device("cuda:0")
    arrays = _edge_inputs(N, seed=N)
    fwd, bwd, near = _reference64(*arrays)
    rows = np.flatnonzero(near["rows"])
    if N > 4:  # the CPU reference's own branches: row 3 clamps, row 4 normalizes
        assert rows.tolist() == [3, 4] and not near["normalized"][3] and near["normalized"][4]
    else:
        assert rows.size == 0
    assert rows.size <= 2
    s, o, q, gs, go, gq = (torch.from_numpy(a).to(dev) for a in arrays)
    leaves = [t.clone().requires_grad_(True) for t in (s, o, q)]
    outs = GaussianActivations.apply(*leaves)
    torch.autograd.backward(outs, [gs, go, gq])
    torch.cuda.synchronize()
    worst = {}
    for (name, (ref, tol)), got in zip(fwd.items(), outs):
        worst[name] = _assert_within(name, got.detach().cpu().numpy(), ref, tol)
    for (name, (ref, tol)), leaf in zip(bwd.items(), leaves):
        worst[name] = _assert_within(name, leaf.grad.cpu().numpy(), ref, tol, near["rows"] if name == "d_rotation"
                                     else None)
    got = leaves[2].grad.cpu().numpy().astype(np.float64)
    for r in rows:  # either branch, whole row
        assert any((np.abs(got[r] - near[b][0][r]) <= near[b][1][r]).all() for b in ("full", "clamp")), \
            f"d_rotation row {r} (|q| within 1e-3 of eps) matches neither branch: {got[r]!r}"
    print(f"activations N={N}: worst err/bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_activations_reject_bad_inputs():
    from gaussian_splatting_lightning_amd.activations import activate
    dev = torch.device("cuda:0")
    s, o, q = _raw(64, 1, dev)
    with pytest.raises(ValueError):
        activate(s, o, q[:, :3].contiguous())
    with pytest.raises(ValueError):
        activate(s.double(), o, q)
    # rotation storage 4 B past a 16-B boundary: the library refuses it rather than misreading
    buf = torch.empty(64 * 4 + 1, device=dev)
    qm = buf[1:].view(64, 4)
    qm.copy_(q)
    with pytest.raises(RuntimeError):
        activate(s, o, qm)
