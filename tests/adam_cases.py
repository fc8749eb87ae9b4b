"""Float64 references, derived per-element bounds and input cases for the optimizer kernels (csrc/gsr_adam.hip).

Pure numpy CPU code, shared by tests/test_adam_host.py (which checks this checker) and tests/test_adam.py (which
holds adam_kernel / sparse_adam_kernel to it on the GPU).  Every check is ONE step from a given fp32 state: the
reference restarts from that state in float64, so the bound is a few fp32 roundings of one update and nothing
accumulates.

Bounds (adam_bounds / sparse_adam_bounds), per element, with e = 2^-24 the largest relative error of one fp32
rounding to nearest:
  m'   2e (|(1-b1)(g-m)| + |m'|): (1-b1) as a float and g-m rounded once each (both scale the first term), the fma's
       rounding (e |m'|), doubled.
  v'   2e (|b2 v| + 2 |(1-b2) g^2|) + 2^-149: b2 as a float (e |b2 v|); (1-b2) as a float, g*g and its product with
       (1-b2) rounded (3e on the second term); the fma's rounding (e |v'| <= e (|b2 v| + |(1-b2) g^2|)).  2^-149 is
       one subnormal quantum: where g*g or v' is subnormal its roundings are absolute, half a quantum each.
       The dense step adds e |b2 v|: adam_update rounds v b2 on its own, as torch's mul_(beta2) does, before the fma
       (which then takes (1-b2) (g g) unrounded: the budget of the second term is not used up, and stays).  Without
       that term the fp32 evaluation of tests/test_adam_host.py leaves the bound by 6 % where g^2 is small against v.
  p'   the float64 update u(m, v) = step_size m / (sqrt(v) / sqrt(bc2) + eps) is monotone in m and in v, so over the
       box (m' +- tol_m) x (max(v' +- tol_v, 0)) it lies between its values at the four corners; the kernel's own m'
       and v' are inside that box.  On top: 4e |u| for the sqrt, the two divides and the fma, and e |p'| for the final
       rounding of p.  With p = 0 the last term is part of the 4e |u| already counted, but it stays: then the whole
       bound is a few ulp of the update.
The sparse step has no bias correction: u = lr m / (sqrt(v) + eps).  Its moments take the same two expressions although
sparse_adam_one computes m' = b1 m + b1c g, not the lerp: b1 and b1c = 1 - b1 are exact inputs with b1 + b1c = 1, so
m' = m + D with D = b1c (g - m) and m = m' - D, hence |b1 m| <= b1 (|m'| + |D|) and |b1c g| = |D + b1c m| <=
(1 + b1c) |D| + b1c |m'|.  The roundings are those of the two products and of the sum, e (|b1 m| + |b1c g| + |m'|)
<= e ((b1 + 1 + b1c) |D| + (b1 + b1c + 1) |m'|) = 2e (|D| + |m'|): the same bound, reached only with no product
fused into the sum (the compiler fuses one: tests/test_adam_host.py evaluates all three forms).  v' = b2 v + (b2c g) g
has the dense form's roundings less those of the two constants.
"""
from __future__ import annotations

import math

import numpy as np

EPS32 = 2.0 ** -24       # one fp32 rounding to nearest, relative
QUANTUM = 2.0 ** -149    # the smallest fp32 subnormal
MIN_NORMAL = 2.0 ** -126

# gradient magnitudes: 0; 1e-30 and 1e-22 (g*g underflows); 1e-19 (g*g at the smallest normal); 1e-17 (g*g normal,
# its root still below eps = 1e-15); everyday values; 1e15 (g*g still finite)
LADDER = (0.0, 1e-30, 1e-22, 1e-19, 1e-17, 1e-10, 1e-4, 1.0, 1e4, 1e15)
# the order the rungs are laid over consecutive elements: every rung once, the three everyday ones twice.  13 is
# coprime to 4 and 1024, so every rung lands on every lane of a float4 and every thread of a workgroup slice.
_RUNG_CYCLE = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 6, 7, 8)
# exp_avg_sq before the step: "one" ~ 1, "g2" ~ g*g, "zero", "sub" a subnormal
_V_CYCLE = ("one", "g2", "one", "zero", "one", "one", "g2", "sub")
_PERIOD = len(_RUNG_CYCLE) * len(_V_CYCLE)   # 104 elements: every (rung, v0 kind) pair once


def f64(a) -> np.ndarray:
    return np.asarray(a, dtype=np.float64)


# ------------------------------------------------------------------------------------------------ references


def _bias(lr, b1, b2, t):
    bc1 = 1.0 - b1 ** t
    bc2 = 1.0 - b2 ** t
    return lr / bc1, math.sqrt(bc2)


def _update(m, v, step_size, bc2_sqrt, eps):
    return step_size * m / (np.sqrt(v) / bc2_sqrt + eps)


def adam_ref64(p, g, m, v, lr, b1, b2, eps, t):
    """One torch-Adam step (non-amsgrad, no weight decay) from fp32 state, all in float64:
    m' = lerp(m, g, 1 - b1);  v' = v b2 + (1 - b2) g^2;  p' = p - step_size m' / (sqrt(v') / sqrt(bc2) + eps)
    with step_size = lr / (1 - b1^t) and bc2 = 1 - b2^t from Python floats.  Returns (p', m', v')."""
    p, g, m, v = f64(p), f64(g), f64(m), f64(v)
    step_size, bc2_sqrt = _bias(float(lr), float(b1), float(b2), int(t))
    m2 = m + (1.0 - b1) * (g - m)
    v2 = v * b2 + (1.0 - b2) * g * g
    return p - _update(m2, v2, step_size, bc2_sqrt, float(eps)), m2, v2


# the upstream kernel takes b1 and b2 as floats and forms 1 - b in float from them (1 - 0.999f = 0.00099998713), and
# so does gsr_sparse_adam_step: the four fp32 values, widened, are inputs of the operation, not roundings of it
SPARSE_B1, SPARSE_B2 = float(np.float32(0.9)), float(np.float32(0.999))
SPARSE_B1C = float(np.float32(1.0) - np.float32(0.9))
SPARSE_B2C = float(np.float32(1.0) - np.float32(0.999))


def _rows(visible, M, shape):
    return np.repeat(np.asarray(visible) != 0, M).reshape(shape)


def sparse_adam_ref64(p, g, m, v, visible, M, lr, eps):
    """SparseGaussianAdam.step in float64: m' = b1 m + (1-b1) g;  v' = b2 v + (1-b2) g^2;  p' = p - lr m' / (sqrt(v')
    + eps) on the elements of visible Gaussians (element e belongs to Gaussian e // M, visible = any nonzero byte),
    the others unchanged.  Returns (p', m', v')."""
    p, g, m, v = f64(p), f64(g), f64(m), f64(v)
    keep = _rows(visible, M, p.shape)
    m2 = SPARSE_B1 * m + SPARSE_B1C * g
    v2 = SPARSE_B2 * v + SPARSE_B2C * g * g
    p2 = p - _update(m2, v2, float(lr), 1.0, float(eps))
    return np.where(keep, p2, p), np.where(keep, m2, m), np.where(keep, v2, v)


# ---------------------------------------------------------------------------------------------------- bounds


def _bounds(p2, m2, v2, tol_m, tol_v, step_size, bc2_sqrt, eps):
    u = _update(m2, v2, step_size, bc2_sqrt, eps)
    span = np.zeros_like(u)
    for sm in (-1.0, 1.0):
        for sv in (-1.0, 1.0):
            corner = _update(m2 + sm * tol_m, np.maximum(v2 + sv * tol_v, 0.0), step_size, bc2_sqrt, eps)
            span = np.maximum(span, np.abs(corner - u))
    tol_p = span + 4.0 * EPS32 * np.abs(u) + EPS32 * np.abs(p2)
    return {"p": tol_p, "m": tol_m, "v": tol_v, "u": u}


def adam_bounds(p, g, m, v, lr, b1, b2, eps, t):
    """Per-element tolerances {"p", "m", "v"} of one adam_kernel step around adam_ref64 (derivation: module
    docstring), and "u", the float64 update itself."""
    p, g, m, v = f64(p), f64(g), f64(m), f64(v)
    p2, m2, v2 = adam_ref64(p, g, m, v, lr, b1, b2, eps, t)
    tol_m = 2.0 * EPS32 * (np.abs((1.0 - b1) * (g - m)) + np.abs(m2))
    tol_v = 2.0 * EPS32 * (np.abs(b2 * v) + 2.0 * np.abs((1.0 - b2) * g * g)) + QUANTUM + EPS32 * np.abs(b2 * v)
    step_size, bc2_sqrt = _bias(float(lr), float(b1), float(b2), int(t))
    return _bounds(p2, m2, v2, tol_m, tol_v, step_size, bc2_sqrt, float(eps))


def sparse_adam_bounds(p, g, m, v, lr, eps):
    """The same for the visible elements of one sparse_adam_kernel step (no bias correction)."""
    p, g, m, v = f64(p), f64(g), f64(m), f64(v)
    p2, m2, v2 = sparse_adam_ref64(p, g, m, v, np.ones(1, np.uint8), p.size, lr, eps)
    tol_m = 2.0 * EPS32 * (np.abs(SPARSE_B1C * (g - m)) + np.abs(m2))
    tol_v = 2.0 * EPS32 * (np.abs(SPARSE_B2 * v) + 2.0 * np.abs(SPARSE_B2C * g * g)) + QUANTUM
    return _bounds(p2, m2, v2, tol_m, tol_v, float(lr), 1.0, float(eps))


def worst_ratio(got, ref, tol, where=None) -> float:
    """max |got - ref| / tol over the elements (of `where`); an element with tol = 0 must be exact (ratio 0 or inf)."""
    err = np.abs(f64(got) - f64(ref)).ravel()
    tol = np.broadcast_to(f64(tol), np.shape(ref)).ravel()
    if where is not None:
        sel = np.asarray(where).ravel()
        err, tol = err[sel], tol[sel]
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / tol)
    return float(np.max(r))


# ----------------------------------------------------------------------------------------------------- cases


def rung_of(n: int, start: int = 0) -> np.ndarray:
    """LADDER index of each of n consecutive elements, the first at case position `start`."""
    j = start + np.arange(n, dtype=np.int64)
    return np.asarray(_RUNG_CYCLE, dtype=np.int64)[j % len(_RUNG_CYCLE)]


def build_case(sizes, seed: int, fresh=()):
    """fp32 state and gradients for parameters of the given element counts: a list of {"p", "g", "m", "v", "rung"}.

    Element j of the case (counted through all its parameters) takes its gradient rung, the kind of its exp_avg_sq
    and whether its parameter is 0 from j alone, so that over every 208 consecutive elements each (rung, v0 kind,
    p0 == 0) combination occurs exactly once; everything else is drawn from `seed`.
      g   = +-rung * [1, 2): both signs; the factor walks 1e-19 across the smallest normal g*g
      p0  = 0 for half of the elements (there p' = -u: the bound is a few ulp of the update), else ~N(0, 1)
      m0  in {0, g (g - m cancels to 0), g (1 + 2^-12) (cancels to a few bits), g / 2, -3 g, sign(g) |N(0, 1e-3)|}
      v0  in {~1, ~g^2 (underflows with g^2), 0, a subnormal}
    Parameters listed in `fresh` (indices) get m0 = v0 = 0: the state GaussianAdam creates on a first step."""
    rng = np.random.default_rng(seed)
    out = []
    start = 0
    for gi, n in enumerate(sizes):
        j = start + np.arange(n, dtype=np.int64)
        start += n
        rung = rung_of(n, int(j[0]) if n else 0)
        mag = np.asarray(LADDER)[rung] * (1.0 + rng.random(n))
        sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
        g = (sign * mag).astype(np.float32)
        p_zero = ((j + j // _PERIOD) % 2) == 0
        p = np.where(p_zero, 0.0, rng.standard_normal(n)).astype(np.float32)
        g64 = g.astype(np.float64)
        mk = rng.integers(0, 6, n)
        m = np.select([mk == 0, mk == 1, mk == 2, mk == 3, mk == 4],
                      [np.zeros(n), g64, g64 * (1.0 + 2.0 ** -12), 0.5 * g64, -3.0 * g64],
                      sign * np.abs(rng.standard_normal(n)) * 1e-3).astype(np.float32)
        vk = np.asarray(_V_CYCLE)[(j // len(_RUNG_CYCLE)) % len(_V_CYCLE)]
        v = np.select([vk == "one", vk == "g2", vk == "zero"],
                      [0.5 + rng.random(n), g64 * g64 * (0.5 + 1.5 * rng.random(n)), np.zeros(n)],
                      rng.integers(1, 2 ** 20, n) * QUANTUM).astype(np.float32)
        if gi in fresh:
            m[:] = 0.0
            v[:] = 0.0
        out.append({"p": p, "g": g, "m": m, "v": v, "rung": rung})
    return out


# the shapes of tests/test_adam.py, here so that tests/test_adam_host.py proves the bound on the very same inputs
TABLE_SIZES = [1, 3, 4, 5, 1023, 1024, 1025, 2048, 4099, 0, 7, 1024, 2, 45 * 33, 16 * 3 * 21, 1, 1024 * 3, 6, 1000]
TABLE_FRESH = (4, 11)            # parameters stepped without any optimizer state yet (t = 1, zero moments)
TABLE_STEP = 7                   # the step the others take
GUARD_SIZES = [5, 1024, 1027]
LATE_STEPS = (1, 2, 1000, 30_000, 1_000_000)
LATE_LRS = (1.6e-4, 0.0, 0.025, 1e-3, 5e-3)
LATE_SIZES = (1027, 1024, 5, 2051, 1000)
LATE_HYPER = ((1e-15, (0.9, 0.999)), (1e-8, (0.5, 0.9)))
LADDER_N = 4099
LADDER_EPS = (1e-15, 1e-8)
LADDER_STEP = 30_000
SPARSE_N = 1027
SPARSE_M = (3, 3, 45, 1, 3, 4)
SPARSE_LRS = (1.6e-4, 2.5e-3, 1.25e-4, 0.025, 5e-3, 1e-3)
# single-parameter groups of the second optimizer (M = 1 + k % 4): 17 at eps = 1e-15, one more than ADAM_MAX_GROUPS,
# so that batch takes two gsr_sparse_adam_step calls (16 + 1), and 4 at eps = 1e-8 (every fifth group)
SPARSE_MANY = 21
SPARSE_MANY_EPS = tuple(1e-8 if k % 5 == 1 else 1e-15 for k in range(SPARSE_MANY))
DEFAULT = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-15)


def dense_cases():
    """name -> list of (state, hyper) per parameter, hyper = dict(lr, b1, b2, eps, t): every dense case of
    tests/test_adam.py."""
    cases = {}
    tab = build_case(TABLE_SIZES, seed=11, fresh=TABLE_FRESH)
    cases["table"] = [(s, dict(DEFAULT, lr=(1.6e-4, 0.025, 1e-3)[i % 3], t=1 if i in TABLE_FRESH else TABLE_STEP))
                      for i, s in enumerate(tab)]
    cases["guard"] = [(s, dict(DEFAULT, lr=0.01, t=3)) for s in build_case(GUARD_SIZES, seed=12)]
    late = build_case(LATE_SIZES * len(LATE_HYPER), seed=13)
    cases["late"] = []
    for h, (eps, (b1, b2)) in enumerate(LATE_HYPER):
        for k, t in enumerate(LATE_STEPS):
            i = h * len(LATE_STEPS) + k
            # the lr list is turned by one in the second batch, so lr = 0 meets two different steps
            cases["late"].append((late[i], dict(lr=LATE_LRS[(k + h) % len(LATE_LRS)], b1=b1, b2=b2, eps=eps, t=t)))
    lad = build_case([LADDER_N] * len(LADDER_EPS), seed=14)
    cases["ladder"] = [(s, dict(DEFAULT, lr=0.01, eps=eps, t=LADDER_STEP)) for s, eps in zip(lad, LADDER_EPS)]
    return cases


def sparse_cases():
    """name -> list of (state, dict(lr, eps, M)) per group: the two optimizers of the sparse tests."""
    six = build_case([SPARSE_N * M for M in SPARSE_M], seed=15)
    many_M = [1 + k % 4 for k in range(SPARSE_MANY)]
    many = build_case([SPARSE_N * M for M in many_M], seed=16)
    return {
        "sparse_six": [(s, dict(lr=lr, eps=1e-15, M=M)) for s, lr, M in zip(six, SPARSE_LRS, SPARSE_M)],
        "sparse_many": [(s, dict(lr=SPARSE_LRS[k % 6], eps=SPARSE_MANY_EPS[k], M=M))
                        for k, (s, M) in enumerate(zip(many, many_M))],
    }


def visibility_patterns(N: int, seed: int = 5):
    """name -> (N,) visibility of the sparse tests: bool patterns and one uint8 with values other than 0 / 1."""
    rng = np.random.default_rng(seed)
    first, last = np.zeros(N, bool), np.zeros(N, bool)
    first[0], last[-1] = True, True
    return {
        "all": np.ones(N, bool), "none": np.zeros(N, bool), "alternating": (np.arange(N) % 2) == 0,
        "first": first, "last": last, "random": rng.random(N) < 0.6,
        "uint8": rng.choice(np.asarray([0, 1, 2, 255], dtype=np.uint8), N),
    }
