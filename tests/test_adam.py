"""adam_kernel and sparse_adam_kernel (csrc/gsr_adam.hip, driven by optim.py) per element against float64.

Every check is one step from a given fp32 state; the float64 reference (tests/adam_cases.py) restarts from that state
and every element of the parameter and of both moments must be within adam_bounds of it -- a few fp32 roundings of
one update, derived there and shown on the CPU by tests/test_adam_host.py to be both sharp and wide enough.  All four
arrays of every parameter live inside larger buffers with guard words on each side, which must come back intact.
The trajectory comparison against torch.optim.Adam stays in tests/test_densify.py.
"""
import numpy as np
import pytest
import torch
from torch import nn

from tests import adam_cases as C
from tests import parity

pytestmark = pytest.mark.gpu

GUARD = 8                 # guard words on each side of every array
SENTINEL = 0x7FA5C3D1     # a NaN's bit pattern: read as a float by mistake it poisons the result as well
ARRAYS = ("param", "grad", "exp_avg", "exp_avg_sq")


class Guarded:
    """values as an fp32 view into a buffer with GUARD sentinel words on each side, `offset` floats (4 B each) past
    16-B alignment."""

    def __init__(self, values: np.ndarray, dev, offset: int = 0, shape=None):
        n = values.size
        self.lo, self.n = GUARD + offset, n
        self.buf = torch.full((self.lo + n + GUARD,), SENTINEL, dtype=torch.int32, device=dev)
        assert self.buf.data_ptr() % 16 == 0
        self.view = self.buf.view(torch.float32)[self.lo:self.lo + n].view(values.shape if shape is None else shape)
        self.view.copy_(torch.from_numpy(np.ascontiguousarray(values)).view(self.view.shape))
        assert n == 0 or self.view.data_ptr() % 16 == 4 * (offset % 4)

    def intact(self) -> bool:
        b = self.buf.cpu().numpy()
        return bool((b[:self.lo] == SENTINEL).all() and (b[self.lo + self.n:] == SENTINEL).all())

    def numpy(self) -> np.ndarray:
        return self.view.detach().cpu().numpy().copy()


def _bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).ravel().view(np.uint32)


def _same_bits(a, b) -> bool:
    return np.array_equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ dense step


def run_dense(dev, groups, offsets=(0, 0, 0, 0), order=None, no_grad=(), fresh=(), grads=None):
    """One GaussianAdam.step() over `groups` (a case of adam_cases.dense_cases: (state, hyper) per parameter, each
    its own param_group), the four arrays of parameter i `offsets` floats past alignment.  `no_grad`: parameters
    without .grad; `fresh`: parameters without optimizer state; `grads`: i -> tensor to use as .grad instead of the
    guarded view.  Returns {i: (p, m, v, step) as numpy} after checking guards, steps and untouched parameters."""
    from gaussian_splatting_lightning_amd.optim import GaussianAdam
    order = list(range(len(groups))) if order is None else list(order)
    arrays, params = {}, {}
    for i in order:
        s, _ = groups[i]
        arrays[i] = {"param": Guarded(s["p"], dev, offsets[0]), "grad": Guarded(s["g"], dev, offsets[1]),
                     "exp_avg": Guarded(s["m"], dev, offsets[2]), "exp_avg_sq": Guarded(s["v"], dev, offsets[3])}
        params[i] = nn.Parameter(arrays[i]["param"].view)
        assert params[i].data_ptr() == arrays[i]["param"].view.data_ptr()
    opt = GaussianAdam([{"params": [params[i]], "lr": groups[i][1]["lr"], "eps": groups[i][1]["eps"],
                         "betas": (groups[i][1]["b1"], groups[i][1]["b2"])} for i in order], lr=0.0)
    for i in order:
        if i not in no_grad:
            if grads is not None and i in grads:
                params[i].grad_dtype = None  # .grad of another dtype than the parameter's
                params[i].grad = grads[i]
            else:
                params[i].grad = arrays[i]["grad"].view
        if i not in fresh:
            opt.state[params[i]] = {"step": torch.tensor(float(groups[i][1]["t"] - 1)),
                                    "exp_avg": arrays[i]["exp_avg"].view, "exp_avg_sq": arrays[i]["exp_avg_sq"].view}
    opt.step()
    torch.cuda.synchronize()
    out = {}
    for i in order:
        s, h = groups[i]
        st = opt.state[params[i]]
        for name, a in arrays[i].items():
            assert a.intact(), f"parameter {i} (n = {s['p'].size}): guard words of {name} overwritten"
        assert _same_bits(arrays[i]["grad"].numpy(), s["g"]), f"parameter {i}: gradient changed"
        if i in no_grad:
            # no gradient: parameter, state (if any) and step stay as they were, bit for bit
            assert _same_bits(arrays[i]["param"].numpy(), s["p"]), f"parameter {i} without a gradient changed"
            if i in fresh:
                assert len(st) == 0
            else:
                assert float(st["step"]) == h["t"] - 1
                assert _same_bits(arrays[i]["exp_avg"].numpy(), s["m"]) and \
                    _same_bits(arrays[i]["exp_avg_sq"].numpy(), s["v"]), f"state of parameter {i} changed"
            continue
        assert float(st["step"]) == h["t"], f"parameter {i}: step {float(st['step'])}, expected {h['t']}"
        if i in fresh:
            m, v = st["exp_avg"].cpu().numpy(), st["exp_avg_sq"].cpu().numpy()
        else:
            assert st["exp_avg"].data_ptr() == arrays[i]["exp_avg"].view.data_ptr()
            m, v = arrays[i]["exp_avg"].numpy(), arrays[i]["exp_avg_sq"].numpy()
        out[i] = (arrays[i]["param"].numpy(), m, v)
    return out


def check_dense(groups, out, label, grad_values=None):
    """Every element of p, exp_avg and exp_avg_sq within adam_bounds of the float64 step; lr = 0 leaves p bitwise.
    Returns the worst err / tol per array."""
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for i, got in out.items():
        s, h = groups[i]
        g = s["g"] if grad_values is None or i not in grad_values else grad_values[i]
        ref = C.adam_ref64(s["p"], g, s["m"], s["v"], **h)
        tol = C.adam_bounds(s["p"], g, s["m"], s["v"], **h)
        for k, a, r in zip(("p", "m", "v"), got, ref):
            ratio = C.worst_ratio(a, r, tol[k])
            worst[k] = max(worst[k], ratio)
            assert ratio <= 1.0, f"{label}: parameter {i} (n = {s['p'].size}, {h}): {k} err / tol = {ratio:.3f}"
        if h["lr"] == 0.0:
            assert _same_bits(got[0], s["p"]), f"{label}: parameter {i}: lr = 0 moved the parameter"
    print(f"{label}: worst err/tol " + ", ".join(f"{k} {x:.3f}" for k, x in worst.items()))
    return worst


@pytest.mark.parametrize("reverse", [False, True], ids=["listed", "reversed"])
def test_group_table_edges(gpu_device, reverse):
    """19 parameters (two gsr_adam_step calls: ADAM_MAX_GROUPS = 16), an empty one in the middle, multiples of the
    1024-element slice followed by tiny groups, n < 4, two parameters without a gradient (one with state, one
    without) and two stepped without state yet; then the same list reversed, so other groups meet the slice
    boundaries."""
    groups = C.dense_cases()["table"]
    assert len(groups) > 16 and 0 in C.TABLE_SIZES
    no_grad = (3, 13)  # n = 5 with state, n = 45 * 33 without
    order = range(len(groups))
    out = run_dense(gpu_device, groups, order=reversed(order) if reverse else order, no_grad=no_grad,
                    fresh=C.TABLE_FRESH + (13,))
    assert sorted(out) == [i for i in order if i not in no_grad]
    worst = check_dense(groups, out, "table/" + ("reversed" if reverse else "listed"))
    parity.record("adam_table", "reversed" if reverse else "listed", worst)


# ---------------------------------------------------------------------------------- guard bands, alignment


@pytest.fixture(scope="module")
def guard_aligned(gpu_device):
    groups = C.dense_cases()["guard"]
    out = run_dense(gpu_device, groups)
    check_dense(groups, out, "guard/aligned")
    return out


_MISALIGNED = [(name, off) for name in ARRAYS for off in (1, 2, 3)]


@pytest.mark.parametrize("which,off", _MISALIGNED + [("all", 0)], ids=lambda x: str(x))
def test_guard_bands_and_alignment(gpu_device, guard_aligned, which, off):
    """Groups of 5, 1024 and 1027 elements with exactly one of the four arrays 1, 2 or 3 floats past 16-B alignment
    (the float4 path is chosen from the OR of the four pointers), or all four (by 1, 2, 3, 2).  Guards intact (in
    run_dense), results within bounds, and bitwise those of the aligned run: the float4 and the scalar branch share
    adam_update with contraction off."""
    offsets = (1, 2, 3, 2) if which == "all" else tuple(off if name == which else 0 for name in ARRAYS)
    groups = C.dense_cases()["guard"]
    out = run_dense(gpu_device, groups, offsets=offsets)
    check_dense(groups, out, f"guard/{which}+{off}")
    for i, got in out.items():
        for k, a, b in zip(("p", "exp_avg", "exp_avg_sq"), got, guard_aligned[i]):
            assert _same_bits(a, b), f"parameter {i}: {k} differs between the aligned and the misaligned run"


def test_non_contiguous_and_half_gradients(gpu_device, guard_aligned):
    """The g.float().contiguous() path of optim.py: a strided gradient (same values: bitwise the aligned run) and an
    fp16 gradient (the reference steps with the fp16 values widened)."""
    groups = C.dense_cases()["guard"]
    strided = {}
    for i, (s, _) in enumerate(groups):
        wide = torch.zeros(2 * s["g"].size, device=gpu_device)
        wide[::2] = torch.from_numpy(s["g"]).to(gpu_device)
        strided[i] = wide[::2]
        assert not strided[i].is_contiguous()
    out = run_dense(gpu_device, groups, grads=strided)
    check_dense(groups, out, "guard/strided grad")
    for i, got in out.items():
        for a, b in zip(got, guard_aligned[i]):
            assert _same_bits(a, b)
    half = {i: np.clip(s["g"], -6e4, 6e4).astype(np.float16) for i, (s, _) in enumerate(groups)}
    out = run_dense(gpu_device, groups, grads={i: torch.from_numpy(h).to(gpu_device) for i, h in half.items()})
    check_dense(groups, out, "guard/fp16 grad", grad_values={i: h.astype(np.float32) for i, h in half.items()})


# ------------------------------------------------------------------------------- late steps, learning rates


def test_late_steps_learning_rates_and_batches(gpu_device):
    """Ten parameters in one step(): steps 1, 2, 1000, 30 000 and 1 000 000 (preset to t - 1) with five learning
    rates, lr = 0 among them, under (eps 1e-15, betas (0.9, 0.999)) and (eps 1e-8, betas (0.5, 0.9)) -- two batches.
    The bias corrections are checked against float64 at every step; lr = 0 leaves p bitwise (check_dense) while
    both moments move."""
    groups = C.dense_cases()["late"]
    assert {h["t"] for _, h in groups} == set(C.LATE_STEPS) and len({(h["eps"], h["b1"]) for _, h in groups}) == 2
    out = run_dense(gpu_device, groups)
    worst = check_dense(groups, out, "late")
    for i, (s, h) in enumerate(groups):
        if h["lr"] == 0.0:
            assert not _same_bits(out[i][1], s["m"]) and not _same_bits(out[i][2], s["v"])
    parity.record("adam_late", "all", worst)


# ---------------------------------------------------------------------------------------- magnitude ladder


def _per_rung(groups, out):
    """LADDER rung -> worst err / tol of (p, m, v) over the elements with that gradient magnitude."""
    table = {}
    for i, got in out.items():
        s, h = groups[i]
        ref = C.adam_ref64(s["p"], s["g"], s["m"], s["v"], **h)
        tol = C.adam_bounds(s["p"], s["g"], s["m"], s["v"], **h)
        for r, mag in enumerate(C.LADDER):
            row = table.setdefault(f"eps={h['eps']:g} |g|~{mag:g}", {})
            for k, a, b in zip(("p", "m", "v"), got, ref):
                row[k] = max(row.get(k, 0.0), C.worst_ratio(a, b, tol[k], where=s["rung"] == r))
    return table


def test_magnitude_ladder(gpu_device):
    """Gradients 0, 1e-30 ... 1e15 (g * g zero, underflowing, subnormal, at the smallest normal, everyday, near
    overflow) against moments of every size, at eps = 1e-15 and 1e-8, step 30 000: every element within bounds, and
    the worst err / tol per rung printed and recorded (tests/parity.py)."""
    groups = C.dense_cases()["ladder"]
    out = run_dense(gpu_device, groups)
    check_dense(groups, out, "ladder")
    table = _per_rung(groups, out)
    for row, w in table.items():
        print(f"ladder {row}: " + ", ".join(f"{k} {x:.3f}" for k, x in w.items()))
    parity.record("adam_ladder", "err_over_tol", table)


def _normal_or_zero(x) -> np.ndarray:
    x = np.abs(C.f64(x))
    return (x == 0.0) | ((x >= 2.0 * C.MIN_NORMAL) & (x < 1e38))


def _all_intermediates_normal(s, h) -> np.ndarray:
    """Elements on which every fp32 intermediate of the step is a normal number or exactly zero (judged on the
    float64 values, with a factor 2 of room above the smallest normal)."""
    p, g, m, v = (C.f64(s[k]) for k in ("p", "g", "m", "v"))
    p2, m2, v2 = C.adam_ref64(p, g, m, v, **h)
    b1, b2 = h["b1"], h["b2"]
    u = p - p2
    denom = np.sqrt(v2) / np.sqrt(1.0 - b2 ** h["t"]) + h["eps"]
    ok = np.ones(p.shape, bool)
    for x in (m, v, g - m, (1 - b1) * (g - m), m2, g * g, (1 - b2) * g * g, (1 - b2) * g, v * b2, v2, np.sqrt(v2),
              denom, m2 / denom, u, p2):
        ok &= _normal_or_zero(x)
    return ok


@pytest.mark.parametrize("foreach", [False, True], ids=["single_tensor", "foreach"])
def test_ladder_bitwise_equals_torch_adam(gpu_device, foreach):
    """gsr_kernels.h states torch's arithmetic with explicit contractions: on the elements where every fp32
    intermediate is normal or zero, one step is bitwise torch.optim.Adam's on the same device."""
    groups = C.dense_cases()["ladder"]
    out = run_dense(gpu_device, groups)
    for i, (s, h) in enumerate(groups):
        p = nn.Parameter(torch.from_numpy(s["p"]).to(gpu_device))
        p.grad = torch.from_numpy(s["g"]).to(gpu_device)
        opt = torch.optim.Adam([p], lr=h["lr"], betas=(h["b1"], h["b2"]), eps=h["eps"], foreach=foreach)
        opt.state[p] = {"step": torch.tensor(float(h["t"] - 1)),
                        "exp_avg": torch.from_numpy(s["m"]).to(gpu_device),
                        "exp_avg_sq": torch.from_numpy(s["v"]).to(gpu_device)}
        opt.step()
        torch.cuda.synchronize()
        sel = _all_intermediates_normal(s, h)
        assert sel.sum() >= 0.4 * sel.size
        theirs = (p.detach().cpu().numpy(), opt.state[p]["exp_avg"].cpu().numpy(),
                  opt.state[p]["exp_avg_sq"].cpu().numpy())
        for k, a, b in zip(("exp_avg", "exp_avg_sq", "p"), (out[i][1], out[i][2], out[i][0]),
                           (theirs[1], theirs[2], theirs[0])):
            diff = (_bits(a) != _bits(b)) & sel
            print(f"bitwise vs torch ({'foreach' if foreach else 'single tensor'}, eps = {h['eps']:g}): {k} differs "
                  f"on {int(diff.sum())} of {int(sel.sum())} elements")
            assert not diff.any(), f"{k}: {int(diff.sum())} elements differ from torch.optim.Adam"


# ----------------------------------------------------------------------------------------------- sparse step


def run_sparse(dev, groups, vis: np.ndarray, grad_offset: int = 0):
    """One SparseGaussianAdam.step(vis, N) over `groups` (a case of adam_cases.sparse_cases), moments preset and all
    four arrays guarded.  Checks the guards, the step counter and, bitwise, every element of an invisible Gaussian;
    returns {i: (p, m, v)}."""
    from diff_gaussian_rasterization import SparseGaussianAdam
    N = C.SPARSE_N
    arrays, params = [], []
    for s, h in groups:
        shape = (N, h["M"])
        arrays.append({"param": Guarded(s["p"], dev, shape=shape), "grad": Guarded(s["g"], dev, grad_offset, shape),
                       "exp_avg": Guarded(s["m"], dev, shape=shape), "exp_avg_sq": Guarded(s["v"], dev, shape=shape)})
        params.append(nn.Parameter(arrays[-1]["param"].view))
    opt = SparseGaussianAdam([{"params": [p], "lr": h["lr"], "eps": h["eps"]} for p, (_, h) in zip(params, groups)],
                             lr=0.0, eps=1e-15)
    for p, a in zip(params, arrays):
        p.grad = a["grad"].view
        opt.state[p] = {"step": torch.tensor(0.0), "exp_avg": a["exp_avg"].view, "exp_avg_sq": a["exp_avg_sq"].view}
    opt.step(torch.from_numpy(vis).to(dev), N)
    torch.cuda.synchronize()
    out = {}
    for i, ((s, h), p, a) in enumerate(zip(groups, params, arrays)):
        for name, arr in a.items():
            assert arr.intact(), f"group {i} (M = {h['M']}): guard words of {name} overwritten"
        assert float(opt.state[p]["step"]) == 0.0  # upstream never advances it
        assert _same_bits(a["grad"].numpy(), s["g"])
        got = (a["param"].numpy().ravel(), a["exp_avg"].numpy().ravel(), a["exp_avg_sq"].numpy().ravel())
        hidden = np.repeat(vis == 0, h["M"])
        for k, x, x0 in zip(("p", "exp_avg", "exp_avg_sq"), got, (s["p"], s["m"], s["v"])):
            assert _same_bits(x[hidden], x0[hidden]), f"group {i} (M = {h['M']}): {k} of an invisible Gaussian changed"
        out[i] = got
    return out


def check_sparse(groups, out, vis, label):
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for i, got in out.items():
        s, h = groups[i]
        ref = C.sparse_adam_ref64(s["p"], s["g"], s["m"], s["v"], vis, h["M"], h["lr"], h["eps"])
        tol = C.sparse_adam_bounds(s["p"], s["g"], s["m"], s["v"], h["lr"], h["eps"])
        shown = np.repeat(vis != 0, h["M"])
        for k, a, r in zip(("p", "m", "v"), got, ref):
            ratio = C.worst_ratio(a, r, tol[k], where=shown)
            worst[k] = max(worst[k], ratio)
            assert ratio <= 1.0, f"{label}: group {i} (M = {h['M']}, eps = {h['eps']:g}): {k} err / tol = {ratio:.3f}"
    print(f"{label}: worst err/tol " + ", ".join(f"{k} {x:.3f}" for k, x in worst.items()))
    return worst


@pytest.mark.parametrize("pattern", ["all", "none", "alternating", "first", "last", "random", "uint8"])
@pytest.mark.parametrize("case", ["sparse_six", "sparse_many"])
def test_sparse_step(gpu_device, case, pattern):
    """N = 1027 Gaussians: the six reference groups (M = 3, 3, 45, 1, 3, 4: a thread's four elements straddle
    Gaussians), and 21 single-parameter groups under two eps values: two by_eps batches, the one of 17 groups split
    by ADAM_MAX_GROUPS = 16 into a full table and a call with the one group left.  Visible elements within bounds of
    the float64 step; every element of an invisible Gaussian -- p and both preset moments, also the ones the float4
    branch writes back -- bitwise unchanged; uint8 visibility counts any nonzero byte."""
    groups = C.sparse_cases()[case]
    if case == "sparse_many":
        batch = sorted(sum(1 for _, h in groups if h["eps"] == eps) for eps in {h["eps"] for _, h in groups})
        assert batch == [4, 17]  # the chunk loop of SparseGaussianAdam.step: 16 + 1, and a second batch
    vis = C.visibility_patterns(C.SPARSE_N)[pattern]
    if pattern == "uint8":
        assert vis.dtype == np.uint8 and set(np.unique(vis)) == {0, 1, 2, 255}
    out = run_sparse(gpu_device, groups, vis)
    worst = check_sparse(groups, out, vis, f"{case}/{pattern}")
    parity.record("adam_" + case, pattern, worst)


def test_sparse_step_misaligned_gradient(gpu_device):
    """The gradient one float past alignment takes every group through the scalar branch (which skips invisible
    elements instead of writing them back): within bounds, guards intact, invisible elements bitwise."""
    groups = C.sparse_cases()["sparse_six"]
    vis = C.visibility_patterns(C.SPARSE_N)["random"]
    out = run_sparse(gpu_device, groups, vis, grad_offset=1)
    check_sparse(groups, out, vis, "sparse_six/random, grad + 1")
