"""3DGS-MCMC (Kheradmand et al., NeurIPS 2024; gsplat's MCMCStrategy) restated in torch, and the inputs of its tests.

The yardstick of tests/test_mcmc.py and tests/test_mcmc_host.py: the formulas as the paper and gsplat's
compute_relocation / inject_noise_to_position state them, evaluated in the dtype asked for on the fp32 inputs.  float64 is
the truth; the same code in float32 on the CPU gives the error an fp32 evaluation makes, from which the tests form their
bars (bar()).  Nothing here is derived from the HIP kernels: the relocation denominator is the paper's double loop with
math.comb coefficients, the noise builds the 3x3 covariance and multiplies it out.
"""
from __future__ import annotations

import math

import numpy as np
import torch

R_MAX = 51                 # gsplat's binomial table: ratios are clamped to [1, 51]
ULP4 = 4 * 2.0 ** -23      # the floor of every bar: 4 fp32 ulp (4.8e-7 relative)
NOISE_GATE_MIN = 1e-3      # rows whose reference gate reaches this are also compared row by row


def relocation(opacities: torch.Tensor, scales: torch.Tensor, ratios: torch.Tensor, dtype=torch.float64):
    """(o', c, c * scales) of activated opacities (n,), scales (n,3) and integer ratios (n,), in `dtype`:
    o' = 1 - (1 - o)^(1/r), D = sum_{m=1..r} sum_{k=0..m-1} C(m-1,k) (-1)^k / sqrt(k+1) o'^(k+1), c = o / D."""
    o = opacities.to(dtype)
    r = ratios.clamp(1, R_MAX)
    new_o = 1 - torch.pow(1 - o, 1 / r.to(dtype))
    D = torch.zeros_like(o)
    for m in range(1, R_MAX + 1):
        inner = torch.zeros_like(o)
        for k in range(m):
            coeff = math.comb(m - 1, k) * (-1) ** k / math.sqrt(k + 1)
            inner = inner + torch.tensor(coeff, dtype=dtype) * new_o ** (k + 1)
        D = D + torch.where(r >= m, inner, torch.zeros_like(inner))
    c = o / D
    return new_o, c, c[:, None] * scales.to(dtype)


def relocation_closed_form(opacities: torch.Tensor, ratios: torch.Tensor, dtype=torch.float64):
    """The same D through the hockey-stick identity sum_{m=k+1..r} C(m-1,k) = C(r,k+1):
    D = sum_{k=0..r-1} C(r,k+1) (-1)^k o'^(k+1) / sqrt(k+1).  Returns (o', D)."""
    o = opacities.to(dtype)
    r = ratios.clamp(1, R_MAX)
    new_o = 1 - torch.pow(1 - o, 1 / r.to(dtype))
    D = torch.zeros_like(o)
    for k in range(R_MAX):
        coeff = torch.tensor([math.comb(int(ri), k + 1) * (-1) ** k / math.sqrt(k + 1) for ri in r.tolist()], dtype=dtype)
        D = D + coeff * new_o ** (k + 1)
    return new_o, D


def quaternion_matrix(q: torch.Tensor) -> torch.Tensor:
    """R(q) (n,3,3) of unit quaternions (w,x,y,z)."""
    w, x, y, z = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).view(-1, 3, 3)


def noise(opacity: torch.Tensor, scaling: torch.Tensor, rotation: torch.Tensor, z: torch.Tensor, scale: float,
          dtype=torch.float64):
    """(update (N,3), gate (N,)) of the raw parameters opacity (N,1) logit, scaling (N,3) log, rotation (N,4):
    Sigma = R diag(s^2) R^T, gate = 1 / (1 + exp(-100 ((1 - o) - 0.995))), update = Sigma (z gate scale)."""
    o = torch.sigmoid(opacity.to(dtype)).reshape(-1)
    s = torch.exp(scaling.to(dtype))
    q = rotation.to(dtype)
    q = q / q.norm(dim=1, keepdim=True).clamp_min(1e-12)
    R = quaternion_matrix(q)
    cov = R @ torch.diag_embed(s * s) @ R.transpose(1, 2)
    gate = 1 / (1 + torch.exp(-100 * ((1 - o) - 0.995)))
    v = z.to(dtype) * gate[:, None] * torch.tensor(scale, dtype=dtype)
    return torch.bmm(cov, v[:, :, None]).squeeze(-1), gate


def bar(fp32_error: float) -> float:
    """The bar of a measure: twice the error the fp32 restatement makes on the same inputs, at least 4 ulp."""
    return max(2.0 * float(fp32_error), ULP4)


def max_rel(got: torch.Tensor, want: torch.Tensor) -> float:
    got, want = got.double(), want.double()
    return float(((got - want).abs() / want.abs()).max())


def rel_l2(got: torch.Tensor, want: torch.Tensor) -> float:
    got, want = got.double(), want.double()
    return float((got - want).norm() / want.norm())


def max_row_rel(got: torch.Tensor, want: torch.Tensor, rows: torch.Tensor) -> float:
    """Largest |row difference| / |row| over the selected rows (0 when none is selected)."""
    if not bool(rows.any()):
        return 0.0
    got, want = got.double()[rows], want.double()[rows]
    return float(((got - want).norm(dim=1) / want.norm(dim=1)).max())


# ---- inputs ----
RELOCATION_N = 257
RELOCATION_RATIOS = (1, 2, 8, 51, 60)  # 60 is clamped to 51


def relocation_inputs(case: str, n: int = RELOCATION_N):
    """(opacities (n,), scales (n,3), ratios (n,) int32) of one opacity range; the ratios cycle through
    RELOCATION_RATIOS so every range meets every ratio."""
    rng = np.random.default_rng({"low": 1, "high": 2, "one": 3}[case])
    if case == "low":
        o = rng.uniform(0.005, 0.5, n)
        o[:2] = (0.005, 0.5)
    elif case == "high":
        o = 0.99 + rng.uniform(-0.005, 0.005, n)
    else:
        o = 1.0 - rng.uniform(2.0 ** -24, 1e-6, n)
        o[0] = 1.0 - 2.0 ** -24  # the largest fp32 below one
    o = o.astype(np.float32)
    assert (o < 1).all() and (o > 0).all()
    s = np.exp(rng.uniform(np.log(0.001), np.log(0.5), (n, 3))).astype(np.float32)
    r = np.array([RELOCATION_RATIOS[j % len(RELOCATION_RATIOS)] for j in range(n)], dtype=np.int32)
    return torch.tensor(o), torch.tensor(s), torch.tensor(r)


NOISE_SIZES = (1, 63, 257)
NOISE_SCALE = 1.6e-4 * 5e5  # xyz learning rate x gsplat's noise learning rate


def noise_inputs(N: int):
    """Raw (opacity (N,1), scaling (N,3), rotation (N,4), z (N,3)).  Opacities: rows 3k within +-20 % of 0.005 (the gate
    is between 0.475 and 0.525 there), rows 3k+1 at 0.5 (a gate of 3e-22), rows 3k+2 spread over (0.001, 0.02).  Row 0 is
    of the first kind, so N = 1 has a live gate; at N = 257 that is 86 rows.  Quaternions are unnormalised with norms
    from 0.1 to 10; row 0, whose gate is live, has norm 1e-3."""
    rng = np.random.default_rng(100 + N)
    o = np.empty(N)
    o[0::3] = 0.005 * rng.uniform(0.8, 1.2, len(o[0::3]))
    o[1::3] = 0.5
    o[2::3] = np.exp(rng.uniform(np.log(0.001), np.log(0.02), len(o[2::3])))
    opacity = np.log(o / (1 - o)).astype(np.float32).reshape(N, 1)
    scaling = rng.uniform(np.log(0.005), np.log(0.5), (N, 3)).astype(np.float32)
    q = rng.normal(size=(N, 4))
    q *= (10.0 ** rng.uniform(-1, 1, (N, 1))) / np.linalg.norm(q, axis=1, keepdims=True)
    q[0] *= 1e-3 / np.linalg.norm(q[0])
    z = rng.normal(size=(N, 3)).astype(np.float32)
    return (torch.tensor(opacity), torch.tensor(scaling), torch.tensor(q.astype(np.float32)), torch.tensor(z))


PARAMETER_NAMES = ("xyz", "features_dc", "features_rest", "opacity", "scaling", "rotation")
STAT_NAMES = ("max_radii2D", "xyz_grad_accum", "xyz_grad_count")


def scene(N: int, seed: int = 0, dead: int = 0, rest: int = 15):
    """Parameters and statistics of N Gaussians as numpy arrays; the first `dead` rows have opacity 0.001 to 0.004
    (dead under min_opacity 0.005), every other row 0.02 to 0.98."""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    o = rng.uniform(0.02, 0.98, N)
    o[:dead] = rng.uniform(0.001, 0.004, dead)
    p = dict(xyz=rng.normal(size=(N, 3)).astype(f32),
             features_dc=rng.normal(size=(N, 1, 3)).astype(f32),
             features_rest=rng.normal(size=(N, rest, 3)).astype(f32),
             opacity=np.log(o / (1 - o)).astype(f32).reshape(N, 1),
             scaling=rng.uniform(np.log(0.001), np.log(0.5), (N, 3)).astype(f32),
             rotation=rng.normal(size=(N, 4)).astype(f32))
    s = dict(max_radii2D=rng.uniform(1, 40, N).astype(f32), xyz_grad_accum=rng.uniform(1e-5, 1e-3, N).astype(f32),
             xyz_grad_count=rng.integers(1, 6, N).astype(f32))
    return p, s


def raw_relocation(opacity: torch.Tensor, scaling: torch.Tensor, src: torch.Tensor, min_opacity: float):
    """The new raw (opacity (n,), scaling (n,3)) of the source rows `src` in float64: ratio from the occurrences of
    each row in src, o' clamped to [min_opacity, 1 - 2^-23], then logit and log."""
    N = opacity.shape[0]
    ratios = 1 + torch.bincount(src, minlength=N)[src]
    o = torch.sigmoid(opacity.double().reshape(-1))[src]
    s = torch.exp(scaling.double())[src]
    new_o, _, new_s = relocation(o, s, ratios.to(torch.int32))
    new_o = new_o.clamp(min_opacity, 1 - 2.0 ** -23)
    return torch.log(new_o / (1 - new_o)), torch.log(new_s)
