"""CPU checks of the checker of tests/test_adam.py (tests/adam_cases.py): no GPU, no HIP library.

  * adam_ref64 is torch.optim.Adam: float64 against float64 at steps 1 ... 1 000 000.
  * sparse_adam_ref64 is the restatement of the upstream sparse kernel (tests/test_densify.py), in float64.
  * the bound has teeth: on the elements whose parameter starts at 0 it is a few ulp of the update.
  * the bound is not too tight: the kernels' formulas evaluated in numpy float32, in the kernels' operation order,
    stay inside it on every element of every case the GPU tests run.
"""
import numpy as np
import pytest
import torch

from tests import adam_cases as C

F32 = np.float32


# ------------------------------------------------------------------------------------- reference vs torch


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.5, 0.9)])
@pytest.mark.parametrize("eps", [1e-15, 1e-8])
@pytest.mark.parametrize("t", [1, 2, 10, 1000, 29_999, 30_000, 1_000_000])
def test_adam_ref64_matches_torch_adam_float64(t, eps, betas):
    """Both sides are about ten float64 roundings (1e-15) of the same formula; 1e-12 relative, no absolute term,
    leaves room for another operation order and nothing else."""
    s = C.build_case([1300], seed=100 + t % 97)[0]
    lr = 0.01
    p = torch.nn.Parameter(torch.tensor(s["p"], dtype=torch.float64))
    p.grad = torch.tensor(s["g"], dtype=torch.float64)
    opt = torch.optim.Adam([p], lr=lr, betas=betas, eps=eps, foreach=False)
    opt.state[p] = {"step": torch.tensor(float(t - 1)), "exp_avg": torch.tensor(s["m"], dtype=torch.float64),
                    "exp_avg_sq": torch.tensor(s["v"], dtype=torch.float64)}
    opt.step()
    assert float(opt.state[p]["step"]) == t
    p2, m2, v2 = C.adam_ref64(s["p"], s["g"], s["m"], s["v"], lr, betas[0], betas[1], eps, t)
    for name, ours, theirs in (("p", p2, p.detach()), ("exp_avg", m2, opt.state[p]["exp_avg"]),
                               ("exp_avg_sq", v2, opt.state[p]["exp_avg_sq"])):
        torch.testing.assert_close(torch.from_numpy(ours), theirs, rtol=1e-12, atol=0.0, msg=lambda m: f"{name}: {m}")


@pytest.mark.parametrize("pattern", ["all", "random", "uint8"])
def test_sparse_ref64_matches_restatement_in_float64(pattern):
    from tests.test_densify import sparse_adam_restatement
    N, M = 301, 3
    s = C.build_case([N * M], seed=7)[0]
    vis = C.visibility_patterns(N)[pattern]
    t64 = [torch.tensor(s[k], dtype=torch.float64).view(N, M) for k in ("p", "g", "m", "v")]
    theirs = sparse_adam_restatement(*t64, torch.from_numpy(vis != 0), M, 0.01, 1e-15)
    ours = C.sparse_adam_ref64(*[s[k].reshape(N, M) for k in ("p", "g", "m", "v")], vis, M, 0.01, 1e-15)
    for name, a, b in zip(("p", "exp_avg", "exp_avg_sq"), ours, theirs):
        assert b.dtype == torch.float64
        torch.testing.assert_close(torch.from_numpy(a), b, rtol=1e-12, atol=0.0, msg=lambda m: f"{name}: {m}")
    hidden = np.repeat(vis == 0, M).reshape(N, M)
    for a, k in zip(ours, ("p", "m", "v")):
        assert np.array_equal(a[hidden], s[k].reshape(N, M).astype(np.float64)[hidden])


# ------------------------------------------------------------------------------------------------ the cases


def _all_cases():
    """name -> list of (state, bounds, lr): every case of tests/test_adam.py with its bounds."""
    out = {}
    for name, groups in C.dense_cases().items():
        out[name] = [(s, C.adam_bounds(s["p"], s["g"], s["m"], s["v"], **h), h) for s, h in groups]
    for name, groups in C.sparse_cases().items():
        out[name] = [(s, C.sparse_adam_bounds(s["p"], s["g"], s["m"], s["v"], h["lr"], h["eps"]), h)
                     for s, h in groups]
    return out


CASES = _all_cases()


def _ref(name, s, h):
    if name.startswith("sparse"):
        return C.sparse_adam_ref64(s["p"], s["g"], s["m"], s["v"], np.ones(1, np.uint8), s["p"].size, h["lr"],
                                   h["eps"])
    return C.adam_ref64(s["p"], s["g"], s["m"], s["v"], **h)


@pytest.mark.parametrize("name", sorted(CASES))
def test_bound_is_a_few_ulp_of_the_update(name):
    """Teeth of the bound, on the reference alone.  Where the parameter starts at 0, the gradient is not 0 and v' is
    a normal fp32 number, tol_p / |u| must be at most 2e-6 (~16 ulp of the update), and those elements must be at
    least 40 % of the case.  A group with lr = 0 has u = 0 and tol_p = 0 on those elements -- its parameters must
    come back bitwise -- so the ratio is undefined there: such a group is left out of both counts."""
    sharp = total = 0
    worst = 0.0
    for s, b, h in CASES[name]:
        _, _, v2 = _ref(name, s, h)
        sel = (s["p"] == 0) & (s["g"] != 0) & (v2 >= C.MIN_NORMAL)
        u, tol = np.abs(b["u"][sel]), b["p"][sel]
        if h["lr"] == 0.0:
            assert not tol.any() and not u.any()
            continue
        assert (u > 0).all()
        worst = max(worst, float((tol / u).max(initial=0.0)))
        sharp += int(sel.sum())
        total += sel.size
    print(f"{name}: worst tol_p/|u| = {worst:.3e} over {sharp} of {total} elements ({100.0 * sharp / total:.1f} %)")
    assert worst <= 2e-6
    assert sharp >= 0.4 * total


# ------------------------------------------------------------------------- fp32 evaluation inside the bound


def _fma(a, b, c):
    """fp32 fma: the product of two floats is exact in float64, so this rounds the sum twice (to 53 bits, then 24) --
    the float64 rounding moves the result by 2^-29 ulp at most."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def adam_fp32(p, g, m, v, lr, b1, b2, eps, t):
    """adam_update of csrc/gsr_kernels.h, operation by operation, with the constants gsr_adam_step hands it."""
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    b1c, b2f, b2c = F32(1.0 - b1), F32(b2), F32(1.0 - b2)
    step_size, bc2_sqrt, epsf = F32(lr / bc1), F32(np.sqrt(bc2)), F32(eps)
    m2 = _fma(np.full_like(m, b1c), g - m, m)
    v2 = _fma(np.full_like(v, b2c), g * g, v * b2f)
    denom = np.sqrt(v2) / bc2_sqrt + epsf
    p2 = _fma(np.full_like(p, -step_size), m2 / denom, p)
    return p2, m2, v2


def sparse_adam_fp32(p, g, m, v, lr, eps, contract):
    """sparse_adam_one of csrc/gsr_adam.hip: b1 * m + b1c * g;  b2 * v + b2c * g * g;  p += -lr * m / (sqrt(v) + eps).
    The source leaves contraction to the compiler: contract = 0 none, 1 the first product of each sum fused, 2 the
    second."""
    b1, b2 = F32(0.9), F32(0.999)
    b1c, b2c = F32(1.0) - b1, F32(1.0) - b2
    lrf, epsf = F32(lr), F32(eps)
    full = np.full_like
    if contract == 0:
        m2 = b1 * m + b1c * g
        v2 = b2 * v + b2c * g * g
    elif contract == 1:
        m2 = _fma(full(m, b1), m, b1c * g)
        v2 = _fma(full(v, b2), v, b2c * g * g)
    else:
        m2 = _fma(full(g, b1c), g, b1 * m)
        v2 = _fma(b2c * g, g, b2 * v)
    q = -lrf * m2 / (np.sqrt(v2) + epsf)
    return p + q, m2, v2


@pytest.mark.parametrize("name", sorted(CASES))
def test_fp32_evaluation_stays_inside_the_bound(name):
    """A correct kernel passes: the same formulas in numpy float32 (IEEE, subnormals kept), in the kernel's operation
    order, are within adam_bounds of the float64 reference on every element of every case."""
    variants = (0, 1, 2) if name.startswith("sparse") else (None,)
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    with np.errstate(under="ignore"):
        for s, b, h in CASES[name]:
            ref = _ref(name, s, h)
            for c in variants:
                if c is None:
                    got = adam_fp32(s["p"], s["g"], s["m"], s["v"], **h)
                else:
                    got = sparse_adam_fp32(s["p"], s["g"], s["m"], s["v"], h["lr"], h["eps"], c)
                for k, a, r in zip(("p", "m", "v"), got, ref):
                    assert a.dtype == F32
                    worst[k] = max(worst[k], C.worst_ratio(a, r, b[k]))
    print(f"{name}: worst err/tol of the fp32 evaluation: " + ", ".join(f"{k} {x:.3f}" for k, x in worst.items()))
    assert max(worst.values()) <= 1.0


def test_cases_cover_the_ladder_at_every_lane():
    """Every rung with both signs lands on every float4 lane of a 4099-element group, and the late-step case meets
    lr = 0 in both batches."""
    s = C.dense_cases()["ladder"][0][0]
    for r in range(len(C.LADDER)):
        for lane in range(4):
            sel = (s["rung"] == r) & (np.arange(s["g"].size) % 4 == lane)
            assert sel.any()
            if r:
                assert (s["g"][sel] > 0).any() and (s["g"][sel] < 0).any()
        slot = np.arange(s["g"].size)[s["rung"] == r] % 1024
        assert np.unique(slot).size >= 250  # 4099 / 13 ~ 315 elements per rung: nearly as many distinct threads
    g2 = s["g"][s["rung"] == 3].astype(np.float64) ** 2
    assert (g2 < C.MIN_NORMAL).any() and (g2 >= C.MIN_NORMAL).any()  # 1e-19: g*g on both sides of the smallest normal
    late = C.dense_cases()["late"]
    assert sorted(h["t"] for _, h in late if h["lr"] == 0.0) == [1, 2]
