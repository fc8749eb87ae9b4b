"""3DGS-MCMC on the GPU (csrc/gsr_mcmc.hip through densify.py): relocation values and noise against the float64
restatement of tests/mcmc_cases.py, and the row moves of relocate_dead / add_new bit for bit.

Bars.  Every error is taken against the float64 restatement on the fp32 inputs; its bar is twice the error the same
restatement makes in fp32 torch on the CPU on the same inputs (computed here, every run), at least 4 fp32 ulp (4.8e-7):
MC.bar.  Achieved errors and bars are recorded through tests.parity (profiles/parity_mcmc.json is one run).

The issue asks for relocate_dead at 40 dead rows with one source repeated 60 times; 40 draws cannot repeat anything 60
times, so the case runs twice: 40 dead rows (one source 30 times, one 3 times) and 70 dead rows (60 times, which the
ratio clamp turns into 51, and 3 times).
"""
import numpy as np
import pytest
import torch
from torch import nn

from tests import mcmc_cases as MC
from tests import parity

pytestmark = pytest.mark.gpu
NAMES = MC.PARAMETER_NAMES
ULP = 2.0 ** -23


class Model(nn.Module):
    """The attributes of the reference GaussianModel that densification touches."""

    def __init__(self, p, s, device):
        super().__init__()
        for k in NAMES:
            setattr(self, f"_{k}", nn.Parameter(torch.tensor(p[k], device=device)))
        for k, v in s.items():
            self.register_buffer(k, torch.tensor(v, device=device))
        self.spatial_scale = 1.0
        self.contrib_count = self.contrib_wsum = self.contrib_wmax = None


def make(N, dead, dev, seed=0, with_optimizer=True, bright=None):
    """A model of N Gaussians, the first `dead` of them dead, and a GaussianAdam with non-zero moments at step 5.
    bright: a row given opacity 0.9, whose relocation values stay above min_opacity at every ratio."""
    from gaussian_splatting_lightning_amd.optim import GaussianAdam
    p, s = MC.scene(N, seed=seed, dead=dead)
    if bright is not None:
        p["opacity"][bright] = np.float32(np.log(0.9 / 0.1))
    model = Model(p, s, dev)
    if not with_optimizer:
        return model, None
    opt = GaussianAdam([{"params": [getattr(model, f"_{k}")], "lr": 1e-3, "name": k} for k in NAMES], lr=0.0, eps=1e-15)
    rng = np.random.default_rng(seed + 1)
    for k in NAMES:
        prm = getattr(model, f"_{k}")
        opt.state[prm] = dict(step=torch.tensor(5.0),
                              exp_avg=torch.tensor(rng.normal(size=prm.shape).astype(np.float32), device=dev),
                              exp_avg_sq=torch.tensor(rng.uniform(0.1, 1, prm.shape).astype(np.float32), device=dev))
    return model, opt


def snapshot(model, opt):
    out = {k: getattr(model, f"_{k}").detach().clone() for k in NAMES}
    out.update({k: getattr(model, k).clone() for k in MC.STAT_NAMES})
    if opt is not None:
        for k in NAMES:
            st = opt.state[getattr(model, f"_{k}")]
            out[f"m_{k}"], out[f"v_{k}"] = st["exp_avg"].clone(), st["exp_avg_sq"].clone()
    return out


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


def assert_same(a: dict, b: dict):
    assert a.keys() == b.keys()
    for k in a:
        assert same_bits(a[k], b[k]), k


# ---------------------------------------------------------------------------------------- relocation values

@pytest.mark.parametrize("case", ["low", "high", "one"])
def test_relocation_values(gpu_device, case):
    """n = 257, ratios 1, 2, 8, 51 and 60 in every opacity range: o in [0.005, 0.5], o near 0.99, o within 1e-6 of 1.
    Measures: max relative error of o' and of c (through c * scales, one more rounding on either side)."""
    from gaussian_splatting_lightning_amd.densify import mcmc_relocation
    o, s, r = MC.relocation_inputs(case)
    assert len(o) == 257 and set(r.tolist()) == {1, 2, 8, 51, 60}
    want_o, _, want_s = MC.relocation(o, s, r)
    f32_o, _, f32_s = MC.relocation(o, s, r, dtype=torch.float32)
    got_o, got_s = mcmc_relocation(o.to(gpu_device), s.to(gpu_device), r.to(gpu_device))
    assert got_o.shape == o.shape and got_s.shape == s.shape and got_o.dtype == got_s.dtype == torch.float32
    got_o, got_s = got_o.cpu(), got_s.cpu()
    res = {}
    for name, got, f32, want in (("new_opacity", got_o, f32_o, want_o), ("c", got_s, f32_s, want_s)):
        res[name] = dict(error=MC.max_rel(got, want), fp32_restatement=MC.max_rel(f32, want))
        res[name]["bar"] = MC.bar(res[name]["fp32_restatement"])
    print(case, res)
    parity.record(f"mcmc_relocation_{case}", "values", res)
    for name, v in res.items():
        assert v["error"] <= v["bar"], (case, name, v)
    # (n,1) opacities come back (n,1); int64 ratios are taken too
    o2, s2 = mcmc_relocation(o.to(gpu_device)[:, None], s.to(gpu_device), r.to(gpu_device).long())
    assert o2.shape == (257, 1) and same_bits(o2.cpu()[:, 0], got_o) and same_bits(s2.cpu(), got_s)


# ---------------------------------------------------------------------------------------- noise

@pytest.mark.parametrize("N", MC.NOISE_SIZES)
def test_noise(gpu_device, N):
    """N = 1, 63, 257: unnormalised quaternions (row 0 of norm 1e-3), a third of the rows within +-20 % of opacity 0.005
    (86 at N = 257; the gate is 0.475 to 0.525 there), a third at 0.5 where the gate is 3e-22.  Measures: relative L2
    of the whole update, and the largest row-wise relative error over the rows whose reference gate is >= 1e-3.  The update is read off zero means; on other
    means the result is the fp32 sum of the means and that update, bit for bit."""
    from gaussian_splatting_lightning_amd.densify import inject_noise
    op, sc, q, z = MC.noise_inputs(N)
    want, gate = MC.noise(op, sc, q, z, MC.NOISE_SCALE)
    f32, _ = MC.noise(op, sc, q, z, MC.NOISE_SCALE, dtype=torch.float32)
    live = gate >= MC.NOISE_GATE_MIN
    assert int(live.sum()) >= (N + 2) // 3 and (N < 257 or int(((gate > 0.47) & (gate < 0.53)).sum()) >= 64)
    p, s = MC.scene(N, seed=N)
    p.update(opacity=op.numpy(), scaling=sc.numpy(), rotation=q.numpy(), xyz=np.zeros((N, 3), np.float32))
    model = Model(p, s, gpu_device)
    xyz_obj = model._xyz
    inject_noise(model, MC.NOISE_SCALE, noise=z.to(gpu_device))
    assert model._xyz is xyz_obj
    got = model._xyz.detach().cpu()
    res = dict(rel_l2=dict(error=MC.rel_l2(got, want), fp32_restatement=MC.rel_l2(f32, want)),
               row_rel=dict(error=MC.max_row_rel(got, want, live), fp32_restatement=MC.max_row_rel(f32, want, live)))
    for v in res.values():
        v["bar"] = MC.bar(v["fp32_restatement"])
    res["live_rows"] = int(live.sum())
    print(N, res)
    parity.record(f"mcmc_noise_N{N}", "update", res)
    for name in ("rel_l2", "row_rel"):
        assert res[name]["error"] <= res[name]["bar"], (N, name, res[name])
    if N > 1:
        assert float(got[1].abs().max()) < 1e-15  # opacity 0.5: the gate is 3e-22
    # on non-zero means: xyz + update in one fp32 addition; the other parameters untouched
    base = torch.tensor(np.random.default_rng(N).normal(size=(N, 3)).astype(np.float32))
    before = snapshot(model, None)
    model._xyz.data.copy_(base)
    inject_noise(model, MC.NOISE_SCALE, noise=z.to(gpu_device))
    assert same_bits(model._xyz.detach().cpu(), base + got)
    after = snapshot(model, None)
    for k in before:
        assert k == "xyz" or same_bits(before[k], after[k]), k
    # drawn noise: the draw normal_(0, 1) makes with that generator
    model._xyz.data.zero_()
    inject_noise(model, MC.NOISE_SCALE, generator=torch.Generator(device=gpu_device).manual_seed(5))
    drawn = model._xyz.detach().clone()
    zz = torch.empty((N, 3), device=gpu_device).normal_(0, 1, generator=torch.Generator(device=gpu_device).manual_seed(5))
    model._xyz.data.zero_()
    inject_noise(model, MC.NOISE_SCALE, noise=zz)
    assert same_bits(drawn, model._xyz.detach())


# ---------------------------------------------------------------------------------------- relocate_dead

def check_source_values(before, after, src, min_opacity=0.005):
    """The sources' new raw opacity and scaling against the float64 restatement, in activated space.  Bar per element:
    8 ulp for the fp32 chain (sigmoid / exp, expm1 and log1p, the division by D, logit / log), plus the quantisation of
    the stored raw value -- half an ulp of |raw| moves sigmoid(raw) and exp(raw) by up to |raw| 2^-24 relative, taken
    twice."""
    want_o, want_s = MC.raw_relocation(before["opacity"].cpu(), before["scaling"].cpu(), src.cpu(), min_opacity)
    got_o, got_s = after["opacity"].cpu().double()[src.cpu(), 0], after["scaling"].cpu().double()[src.cpu()]
    err_o = (torch.sigmoid(got_o) - torch.sigmoid(want_o)).abs() / torch.sigmoid(want_o)
    err_s = (torch.exp(got_s) - torch.exp(want_s)).abs() / torch.exp(want_s)
    assert bool((err_o <= 8 * ULP + want_o.abs() * ULP).all()), float(err_o.max())
    assert bool((err_s <= 8 * ULP + want_s.abs() * ULP).all()), float(err_s.max())
    return float(err_o.max()), float(err_s.max())


def pinned_sources(n_dead, N, big, dev):
    """n_dead alive source rows: row 100 `big` times, row 250 three times, the rest distinct, shuffled."""
    rest = [r for r in range(n_dead + 7, N) if r not in (100, 250)][: n_dead - big - 3]
    idx = np.array([100] * big + [250] * 3 + rest, dtype=np.int64)
    assert len(idx) == n_dead and idx.min() >= n_dead
    return torch.tensor(np.random.default_rng(9).permutation(idx), device=dev)


@pytest.mark.parametrize("n_dead,big", [(40, 30), (70, 60)])
def test_relocate_dead(gpu_device, n_dead, big):
    from gaussian_splatting_lightning_amd.densify import relocate_dead
    N = 300
    src = pinned_sources(n_dead, N, big, gpu_device)
    runs = []
    for rep in range(2):
        model, opt = make(N, n_dead, gpu_device, bright=100)
        before = snapshot(model, opt)
        objs = {k: getattr(model, f"_{k}") for k in NAMES}
        states = {k: opt.state[objs[k]] for k in NAMES}
        moments = {k: (states[k]["exp_avg"], states[k]["exp_avg_sq"]) for k in NAMES}
        assert relocate_dead(model, 0.005, optimizer=opt, sampled_idx=src) == n_dead
        after = snapshot(model, opt)
        runs.append(after)
        for k in NAMES:  # the same objects: parameters, state dicts, moment tensors, group entries
            assert getattr(model, f"_{k}") is objs[k] and opt.state[objs[k]] is states[k]
            assert states[k]["exp_avg"] is moments[k][0] and states[k]["exp_avg_sq"] is moments[k][1]
            assert [g for g in opt.param_groups if g["name"] == k][0]["params"][0] is objs[k]
            assert float(states[k]["step"]) == 5.0
        assert len(opt.state) == len(NAMES)
    assert_same(runs[0], runs[1])
    after = runs[0]
    dst = torch.arange(n_dead, device=gpu_device)  # MC.scene puts the dead rows first; nonzero() lists them in order
    is_src = torch.zeros(N, dtype=torch.bool, device=gpu_device)
    is_src[src] = True
    is_dst = torch.zeros(N, dtype=torch.bool, device=gpu_device)
    is_dst[dst] = True
    for k in NAMES:
        assert same_bits(after[k][dst], after[k][src]), k                       # destinations: their updated sources
        other = ~is_dst if k not in ("opacity", "scaling") else ~(is_dst | is_src)
        assert same_bits(after[k][other], before[k][other]), k                  # every other row
        for mv in ("m_", "v_"):
            assert not bool(after[mv + k][is_src].any()), k                     # source moments: exactly zero
            assert same_bits(after[mv + k][~is_src], before[mv + k][~is_src]), k  # every other moment, dead rows' too
    for k in MC.STAT_NAMES:
        assert same_bits(after[k], before[k]), k
    assert bool((after["opacity"][is_src] != before["opacity"][is_src]).all())
    errs = check_source_values(before, after, src)
    parity.record(f"mcmc_relocate_dead_{n_dead}", "source_values", dict(opacity_rel=errs[0], scale_rel=errs[1]))
    # the row drawn 60 times has the values of ratio 51 (the clamp), which differ from those of ratio 61 unclamped
    if big == 60:
        o = torch.sigmoid(before["opacity"].cpu().double()[100])
        want51 = MC.relocation(o, torch.ones(1, 3), torch.tensor([51], dtype=torch.int32))[0]
        got = torch.sigmoid(after["opacity"].cpu().double()[100, 0])
        assert abs(float(got / want51) - 1) < 1e-5 and abs(float(got / (1 - (1 - o) ** (1 / 61))) - 1) > 1e-2


def test_relocate_dead_draws_what_torch_draws(gpu_device):
    """No pinned indices, a seeded generator: the sources are alive_rows[torch.multinomial(opacity of the alive rows, n,
    replacement=True)] of that generator state -- the result equals the pinned run on exactly those indices."""
    from gaussian_splatting_lightning_amd.densify import relocate_dead
    N, n_dead = 300, 40
    model, opt = make(N, n_dead, gpu_device, seed=2)
    opac = torch.sigmoid(model._opacity.detach()).reshape(-1)
    alive = (opac > 0.005).nonzero().squeeze(-1)
    assert len(alive) == N - n_dead
    pick = torch.multinomial(opac[alive], n_dead, replacement=True,
                             generator=torch.Generator(device=gpu_device).manual_seed(11))
    assert relocate_dead(model, optimizer=opt, generator=torch.Generator(device=gpu_device).manual_seed(11)) == n_dead
    pinned, opt2 = make(N, n_dead, gpu_device, seed=2)
    assert relocate_dead(pinned, optimizer=opt2, sampled_idx=alive[pick]) == n_dead
    assert_same(snapshot(model, opt), snapshot(pinned, opt2))
    other, opt3 = make(N, n_dead, gpu_device, seed=2)
    relocate_dead(other, optimizer=opt3, generator=torch.Generator(device=gpu_device).manual_seed(12))
    assert not same_bits(snapshot(other, opt3)["xyz"], snapshot(model, opt)["xyz"])  # another seed, other sources


def test_relocate_dead_no_ops(gpu_device):
    """No dead row, every row dead, N = 1 (either way): 0 is returned and nothing changes."""
    from gaussian_splatting_lightning_amd.densify import relocate_dead
    for N, dead in ((300, 0), (300, 300), (1, 0), (1, 1)):
        model, opt = make(N, dead, gpu_device)
        before = snapshot(model, opt)
        assert relocate_dead(model, optimizer=opt, generator=torch.Generator(device=gpu_device).manual_seed(1)) == 0
        assert_same(before, snapshot(model, opt))


# ---------------------------------------------------------------------------------------- add_new

def test_add_new(gpu_device):
    from gaussian_splatting_lightning_amd.densify import add_new
    from gaussian_splatting_lightning_amd.optim import GaussianAdam
    N = 300
    src = torch.tensor([5, 17, 5, 299, 0, 5, 17, 123, 44, 200], device=gpu_device)
    model, opt = make(N, 0, gpu_device)
    model.contrib_wmax = torch.ones(N, device=gpu_device)
    before = snapshot(model, opt)
    old = {k: getattr(model, f"_{k}") for k in NAMES}
    assert add_new(model, 310, optimizer=opt, sampled_idx=src) == 10
    after = snapshot(model, opt)
    is_src = torch.zeros(N, dtype=torch.bool, device=gpu_device)
    is_src[src] = True
    for k in NAMES:
        prm = getattr(model, f"_{k}")
        assert isinstance(prm, nn.Parameter) and prm is not old[k] and prm.shape == (310,) + old[k].shape[1:]
        assert same_bits(after[k][N:], after[k][src]), k                           # new rows: their updated sources
        other = torch.ones(N, dtype=torch.bool, device=gpu_device) if k not in ("opacity", "scaling") else ~is_src
        assert same_bits(after[k][:N][other], before[k][other]), k                 # old rows
        for mv in ("m_", "v_"):
            assert same_bits(after[mv + k][:N], before[mv + k]), k                 # old moments, the sources' too
            assert after[mv + k].shape == prm.shape and not bool(after[mv + k][N:].any()), k
        grp = [g for g in opt.param_groups if g["name"] == k][0]
        assert grp["params"][0] is prm and prm in opt.state and old[k] not in opt.state
        assert float(opt.state[prm]["step"]) == 5.0
    assert len(opt.state) == len(NAMES)
    for k in MC.STAT_NAMES:
        assert same_bits(after[k][:N], before[k]) and not bool(after[k][N:].any()), k
    assert model.contrib_wmax is None  # the number of rows changed: the contribution buffers are dropped
    assert bool((after["opacity"][:N][is_src] != before["opacity"][is_src]).all())
    errs = check_source_values(before, after, src)
    parity.record("mcmc_add_new", "source_values", dict(opacity_rel=errs[0], scale_rel=errs[1]))
    # training continues on the rebound optimizer
    for k in NAMES:
        prm = getattr(model, f"_{k}")
        prm.grad = torch.ones_like(prm)
    opt.step()
    torch.cuda.synchronize()
    assert isinstance(opt, GaussianAdam) and float(opt.state[model._xyz]["step"]) == 6.0
    assert bool(torch.isfinite(model._xyz).all()) and not same_bits(model._xyz.detach(), after["xyz"])
    # the cap: nothing is added at cap <= N, and the cap bounds the growth
    for cap in (310, 300, 10):
        assert add_new(model, cap, optimizer=opt) == 0 and model._xyz.shape[0] == 310
    assert add_new(model, 312, optimizer=opt, generator=torch.Generator(device=gpu_device).manual_seed(3)) == 2
    assert model._xyz.shape[0] == 312 and model.max_radii2D.shape[0] == 312


def test_add_new_draws_what_torch_draws(gpu_device):
    from gaussian_splatting_lightning_amd.densify import add_new
    N = 300
    model, opt = make(N, 40, gpu_device, seed=4)
    opac = torch.sigmoid(model._opacity.detach()).reshape(-1)
    pick = torch.multinomial(opac, 15, replacement=True, generator=torch.Generator(device=gpu_device).manual_seed(21))
    assert add_new(model, 10_000, optimizer=opt, generator=torch.Generator(device=gpu_device).manual_seed(21)) == 15
    pinned, opt2 = make(N, 40, gpu_device, seed=4)
    assert add_new(pinned, 10_000, optimizer=opt2, sampled_idx=pick) == 15
    assert_same(snapshot(model, opt), snapshot(pinned, opt2))


# ---------------------------------------------------------------------------------------- determinism

def test_duplicate_sources_are_deterministic(gpu_device):
    """N = 4096, every draw from 8 sources (about 250 copies each, all at the ratio clamp): two calls from the same start
    give the same bits, for the relocation of 2000 dead rows and for a growth of 204 rows."""
    from gaussian_splatting_lightning_amd.densify import add_new, relocate_dead
    N, n_dead = 4096, 2000
    eight = torch.tensor([2048, 2049, 3000, 3001, 3500, 4000, 4094, 4095], device=gpu_device)
    rng = np.random.default_rng(6)
    src_r = eight[torch.tensor(rng.integers(0, 8, n_dead), device=gpu_device)]
    src_a = eight[torch.tensor(rng.integers(0, 8, 204), device=gpu_device)]
    outs = []
    for rep in range(2):
        model, opt = make(N, n_dead, gpu_device, seed=8)
        assert relocate_dead(model, optimizer=opt, sampled_idx=src_r) == n_dead
        a = snapshot(model, opt)
        assert add_new(model, 10 ** 6, optimizer=opt, sampled_idx=src_a) == 204
        outs.append((a, snapshot(model, opt)))
    assert_same(outs[0][0], outs[1][0])
    assert_same(outs[0][1], outs[1][1])
    a = outs[0][0]
    for k in NAMES:  # and all 2000 destinations hold one of the eight updated rows
        assert same_bits(a[k][:n_dead], a[k][src_r]), k
