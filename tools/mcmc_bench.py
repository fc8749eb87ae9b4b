#!/usr/bin/env python
"""Cost of the 3DGS-MCMC operations at bench.py's cfg 3 count (1M Gaussians, SH degree 3), each against the fp32 torch
composition of the same formulas on the same GPU -- the route a user had before csrc/gsr_mcmc.hip.

    python tools/mcmc_bench.py --processes 5 --out profiles/mcmc_cost.json     # five fresh child processes
    python tools/mcmc_bench.py --child                                         # one process, one JSON line
    python tools/mcmc_bench.py --child --only noise_kernel                     # the launch alone (for a kernel trace)

* noise: inject_noise(model, scale, noise=z) with z supplied, and the torch ops of gsplat's inject_noise_to_position
  with the 3x3 products written out as elementwise ops (`noise_torch_ms`, the yardstick) or as torch.bmm
  (`noise_torch_bmm_ms`: a million batched 3x3 products, which rocBLAS runs far slower; 5 blocks of 10 calls).
  5 blocks of 50 calls, device events around each block, after 10 warm-up calls; ms per call per block.
  `noise_launch_ms`: gsr_mcmc_noise through ctypes back to back (2000 launches per block), which the device bounds once
  the kernel outlasts the host's enqueue.  On one set of arrays the 68 MB stay in the 256 MiB Infinity Cache between
  launches; `noise_launch_rotating_ms` cycles over six sets (408 MB), so every launch reads from HBM: the byte rate
  is 68 B per Gaussian over that, against the 6.29 TB/s achievable HBM rate.  The kernel's own time is a kernel
  trace's to give (--only noise_kernel under the profiler; one set of arrays, cache-resident).
* relocation: relocate_dead with 50 000 dead rows and Adam state, drawn (the source draw and its host read-back
  included, on both sides) and pinned (sampled_idx given: the move alone).  One timed call per repetition on restored
  parameters, 2 warm-ups + 7 repetitions.
* growth: add_new at growth 1.05 (50 000 new rows), a fresh model per repetition as the call changes N; 1 warm-up + 5.
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

NAMES = ("xyz", "features_dc", "features_rest", "opacity", "scaling", "rotation")
SHAPES = dict(xyz=(3,), features_dc=(1, 3), features_rest=(15, 3), opacity=(1,), scaling=(3,), rotation=(4,))
HBM_ACHIEVABLE_TBPS = 6.29
NOISE_BYTES_PER_GAUSSIAN = 68  # read opacity 4, scaling 12, rotation 16, z 12, xyz 12; write xyz 12
MIN_OPACITY = 0.005
R_MAX = 51
ROTATE = 6  # sets of noise arrays the rotating launch cycles over (6 x 68 MB at 1M Gaussians)


def make_model(N, n_dead, torch, nn, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)

    class M(nn.Module):
        pass

    m = M()
    for k in NAMES:
        t = torch.randn((N,) + SHAPES[k], device="cuda", generator=g)
        if k == "scaling":
            t = t * 1.5 - 4.5
        if k == "opacity":
            o = torch.rand((N, 1), device="cuda", generator=g) * 0.9 + 0.02
            o[:n_dead] = torch.rand((n_dead, 1), device="cuda", generator=g) * 0.003 + 0.001
            t = torch.log(o / (1 - o))
        setattr(m, f"_{k}", nn.Parameter(t))
    m.max_radii2D = torch.rand(N, device="cuda", generator=g) * 40
    m.xyz_grad_accum = torch.rand(N, device="cuda", generator=g) * 4e-4
    m.xyz_grad_count = torch.ones(N, device="cuda")
    m.spatial_scale = 1.0
    return m


def make_optimizer(m, torch):
    from gaussian_splatting_lightning_amd.optim import GaussianAdam
    opt = GaussianAdam([{"params": [getattr(m, f"_{k}")], "lr": 1e-3, "name": k} for k in NAMES], lr=0.0, eps=1e-15)
    for k in NAMES:
        p = getattr(m, f"_{k}")
        opt.state[p] = dict(step=torch.tensor(1.0), exp_avg=torch.randn_like(p), exp_avg_sq=torch.rand_like(p))
    return opt


def blocks(fn, torch, calls, nblocks=5, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(nblocks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / calls)
    return out


def once(fn, torch):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


# ---- the torch compositions (fp32, the formulas of include/gsrast.h) ----
def torch_noise(m, z, scale, torch):
    o = torch.sigmoid(m._opacity).flatten()
    s = torch.exp(m._scaling)
    w, x, y, zz = torch.nn.functional.normalize(m._rotation, dim=1).unbind(-1)
    R = torch.stack([1 - 2 * (y * y + zz * zz), 2 * (x * y - w * zz), 2 * (x * zz + w * y),
                     2 * (x * y + w * zz), 1 - 2 * (x * x + zz * zz), 2 * (y * zz - w * x),
                     2 * (x * zz - w * y), 2 * (y * zz + w * x), 1 - 2 * (x * x + y * y)], -1).view(-1, 3, 3)
    M = R * s[:, None, :]
    cov = torch.bmm(M, M.transpose(1, 2))
    gate = 1 / (1 + torch.exp(-100 * ((1 - o) - 0.995)))
    v = z * gate[:, None] * scale
    m._xyz.add_(torch.bmm(cov, v[:, :, None]).squeeze(-1))


def torch_noise_elementwise(m, z, scale, torch):
    """The same without batched 3x3 matmuls (rocBLAS runs a million of them slowly): products and row sums written
    out, Sigma v as R (s^2 o (R^T v))."""
    o = torch.sigmoid(m._opacity).flatten()
    s = torch.exp(m._scaling)
    w, x, y, zz = torch.nn.functional.normalize(m._rotation, dim=1).unbind(-1)
    R = torch.stack([1 - 2 * (y * y + zz * zz), 2 * (x * y - w * zz), 2 * (x * zz + w * y),
                     2 * (x * y + w * zz), 1 - 2 * (x * x + zz * zz), 2 * (y * zz - w * x),
                     2 * (x * zz - w * y), 2 * (y * zz + w * x), 1 - 2 * (x * x + y * y)], -1).view(-1, 3, 3)
    gate = 1 / (1 + torch.exp(-100 * ((1 - o) - 0.995)))
    v = z * gate[:, None] * scale
    u = (R * v[:, :, None]).sum(1) * s * s
    m._xyz.add_((R * u[:, None, :]).sum(2))


def relocation_table(torch):
    t = torch.zeros(R_MAX + 1, R_MAX, dtype=torch.float64)
    for r in range(1, R_MAX + 1):
        for k in range(r):
            t[r, k] = math.comb(r, k + 1) * (-1) ** k / math.sqrt(k + 1)
    return t.float().cuda()


def torch_relocation(o, s, ratio, table, torch):
    r = ratio.clamp(1, R_MAX)
    new_o = 1 - torch.pow(1 - o, 1 / r.float())
    powers = torch.cumprod(new_o[:, None].expand(-1, R_MAX), 1)
    D = (table[r] * powers).sum(1)
    return new_o, (o / D)[:, None] * s


def torch_sources(m, src, table, torch):
    """New raw opacity and scaling of the source rows, written in place at the sources."""
    N = m._opacity.shape[0]
    ratio = torch.bincount(src, minlength=N)[src] + 1
    o = torch.sigmoid(m._opacity).flatten()[src]
    new_o, new_s = torch_relocation(o, torch.exp(m._scaling)[src], ratio, table, torch)
    new_o = new_o.clamp(MIN_OPACITY, 1 - 2.0 ** -23)
    m._opacity[src] = torch.log(new_o / (1 - new_o))[:, None]
    m._scaling[src] = torch.log(new_s)


def torch_relocate(m, opt, table, torch, generator=None, sampled_idx=None):
    with torch.no_grad():
        opac = torch.sigmoid(m._opacity).flatten()
        dead = opac <= MIN_OPACITY
        dead_idx = dead.nonzero().squeeze(-1)
        n = len(dead_idx)
        if sampled_idx is None:
            alive = (~dead).nonzero().squeeze(-1)
            sampled_idx = alive[torch.multinomial(opac[alive], n, replacement=True, generator=generator)]
        torch_sources(m, sampled_idx, table, torch)
        for k in NAMES:
            p = getattr(m, f"_{k}")
            p[dead_idx] = p[sampled_idx]
            st = opt.state[p]
            st["exp_avg"][sampled_idx] = 0
            st["exp_avg_sq"][sampled_idx] = 0
    return n


def torch_add(m, opt, table, torch, nn, generator=None):
    with torch.no_grad():
        N = m._xyz.shape[0]
        n = int(1.05 * N) - N
        opac = torch.sigmoid(m._opacity).flatten()
        if N <= 2 ** 24:
            src = torch.multinomial(opac, n, replacement=True, generator=generator)
        else:
            cdf = torch.cumsum(opac.double(), 0)
            src = torch.searchsorted(cdf, torch.rand(n, dtype=torch.float64, device="cuda") * cdf[-1]).clamp_(max=N - 1)
        torch_sources(m, src, table, torch)
        for k in NAMES:
            old = getattr(m, f"_{k}")
            new = nn.Parameter(torch.cat([old, old[src]], 0))
            setattr(m, f"_{k}", new)
            st = opt.state.pop(old)
            for mv in ("exp_avg", "exp_avg_sq"):
                st[mv] = torch.cat([st[mv], torch.zeros((n,) + st[mv].shape[1:], device="cuda")], 0)
            grp = [g for g in opt.param_groups if g["name"] == k][0]
            grp["params"][0] = new
            opt.state[new] = st
        for k in ("max_radii2D", "xyz_grad_accum", "xyz_grad_count"):
            setattr(m, k, torch.cat([getattr(m, k), torch.zeros(n, device="cuda")]))
    return n


def child(N, only):
    import torch
    from torch import nn
    from gaussian_splatting_lightning_amd import _native, densify
    assert torch.cuda.is_available(), "mcmc_bench needs a HIP device: there is no CPU path to time"
    lib = _native.load()
    out = {"N": N}
    n_move = N // 20
    scale = 1.6e-4 * 5e5

    m = make_model(N, 0, torch, nn)
    z = torch.randn(N, 3, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def launch():
        lib.gsr_mcmc_noise(N, m._xyz.data_ptr(), m._opacity.data_ptr(), m._scaling.data_ptr(), m._rotation.data_ptr(),
                           z.data_ptr(), scale, stream)

    if only == "noise_kernel":
        for _ in range(200):
            launch()
        torch.cuda.synchronize()
        print(json.dumps({"N": N, "launches": 200}))
        return
    out["noise_fused_ms"] = blocks(lambda: densify.inject_noise(m, scale, noise=z), torch, 50)
    out["noise_launch_ms"] = blocks(launch, torch, 2000, warmup=100)
    # the same launch cycling over ROTATE sets of arrays, ROTATE x 68 MB in all: more than the 256 MiB Infinity Cache
    # holds, so every launch reads its arrays from HBM, as a training step does after the rasterizer ran
    sets = [m] + [make_model(N, 0, torch, nn, seed=20 + i) for i in range(ROTATE - 1)]
    zs = [z] + [torch.randn(N, 3, device="cuda") for _ in range(ROTATE - 1)]
    ptrs = [(g._xyz.data_ptr(), g._opacity.data_ptr(), g._scaling.data_ptr(), g._rotation.data_ptr(), zz.data_ptr())
            for g, zz in zip(sets, zs)]
    turn = [0]

    def launch_rotating():
        a = ptrs[turn[0] % ROTATE]
        turn[0] += 1
        lib.gsr_mcmc_noise(N, a[0], a[1], a[2], a[3], a[4], scale, stream)

    out["noise_launch_rotating_ms"] = blocks(launch_rotating, torch, 2000, warmup=100)
    del sets, zs
    with torch.no_grad():
        out["noise_torch_ms"] = blocks(lambda: torch_noise_elementwise(m, z, scale, torch), torch, 50)
        out["noise_torch_bmm_ms"] = blocks(lambda: torch_noise(m, z, scale, torch), torch, 10, warmup=2)
    # the two routes on the same means: the same update to fp32 rounding
    with torch.no_grad():
        m._xyz.zero_()
        densify.inject_noise(m, scale, noise=z)
        a = m._xyz.detach().clone()
        m._xyz.zero_()
        torch_noise(m, z, scale, torch)
        out["noise_fused_vs_torch_rel_l2"] = float((a - m._xyz).double().norm() / m._xyz.double().norm())
        b = m._xyz.detach().clone()
        m._xyz.zero_()
        torch_noise_elementwise(m, z, scale, torch)
        out["noise_torch_forms_rel_l2"] = float((b - m._xyz).double().norm() / b.double().norm())
    del m, z

    table = relocation_table(torch)
    m = make_model(N, n_move, torch, nn, seed=1)
    opt = make_optimizer(m, torch)
    saved = {k: getattr(m, f"_{k}").detach().clone() for k in NAMES}
    alive = torch.arange(n_move, N, device="cuda")
    pinned = alive[torch.randint(0, N - n_move, (n_move,), device="cuda")]

    def restore():
        with torch.no_grad():
            for k in NAMES:
                getattr(m, f"_{k}").copy_(saved[k])

    for label, fn in (
            ("relocate_fused_drawn_ms", lambda: densify.relocate_dead(m, MIN_OPACITY, optimizer=opt)),
            ("relocate_torch_drawn_ms", lambda: torch_relocate(m, opt, table, torch)),
            ("relocate_fused_pinned_ms", lambda: densify.relocate_dead(m, MIN_OPACITY, optimizer=opt, sampled_idx=pinned)),
            ("relocate_torch_pinned_ms", lambda: torch_relocate(m, opt, table, torch, sampled_idx=pinned))):
        times = []
        for rep in range(9):
            restore()
            moved = []
            t = once(lambda: moved.append(fn()), torch)
            assert moved[0] == n_move, (label, moved)
            if rep >= 2:
                times.append(t)
        out[label] = times
    out["relocate_rows"] = n_move
    del m, opt, saved

    for label in ("add_fused_ms", "add_torch_ms"):
        times = []
        for rep in range(6):
            m = make_model(N, 0, torch, nn, seed=10 + rep)
            opt = make_optimizer(m, torch)
            if label == "add_fused_ms":
                fn = lambda: densify.add_new(m, 10 ** 9, growth=1.05, min_opacity=MIN_OPACITY, optimizer=opt)  # noqa: E731
            else:
                fn = lambda: torch_add(m, opt, table, torch, nn)  # noqa: E731
            added = []
            t = once(lambda: added.append(fn()), torch)
            assert added[0] == int(1.05 * N) - N and m._xyz.shape[0] == int(1.05 * N), (label, added)
            if rep >= 1:
                times.append(t)
            del m, opt
        out[label] = times
    out["add_rows"] = int(1.05 * N) - N
    print(json.dumps(out))


def summarise(runs):
    keys = [k for k in runs[0] if k.endswith("_ms")]
    res = {}
    for k in keys:
        per_process = [statistics.median(r[k]) for r in runs]
        res[k] = dict(samples=[[round(x, 5) for x in r[k]] for r in runs],
                      process_medians=[round(x, 5) for x in per_process], median=round(statistics.median(per_process), 5),
                      min=round(min(per_process), 5), max=round(max(per_process), 5))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--only", default=None, choices=("noise_kernel",))
    ap.add_argument("--processes", type=int, default=5)
    ap.add_argument("--N", type=int, default=1_000_000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds each child process may take")
    a = ap.parse_args()
    if a.child:
        child(a.N, a.only)
        return
    runs = []
    for _ in range(a.processes):  # this process never opens the GPU: every child starts fresh
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--N", str(a.N)], capture_output=True,
                           text=True, timeout=a.timeout)
        if r.returncode != 0:
            sys.exit(f"a child process failed ({r.returncode}), nothing further is started:\n{r.stdout}\n{r.stderr}")
        runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    res = summarise(runs)
    N = a.N
    med = lambda k: res[k]["median"]  # noqa: E731
    launch_s = med("noise_launch_rotating_ms") * 1e-3
    out = {
        "method": __doc__.split("\n\n", 2)[2].strip() if __doc__ else "",
        "workload": f"{N} Gaussians, SH degree 3 (59 floats each), fp32; {runs[0]['relocate_rows']} relocated rows, "
                    f"{runs[0]['add_rows']} added rows; {a.processes} fresh processes, medians of the process medians",
        "times": res,
        "noise": {
            "bytes": NOISE_BYTES_PER_GAUSSIAN * N,
            "fused_call_ms": med("noise_fused_ms"), "torch_call_ms": med("noise_torch_ms"),
            "torch_bmm_call_ms": med("noise_torch_bmm_ms"),
            "torch_over_fused": round(med("noise_torch_ms") / med("noise_fused_ms"), 2),
            "fused_is_faster": med("noise_fused_ms") < med("noise_torch_ms"),
            "cache_resident_launch_ms": med("noise_launch_ms"),
            "cache_resident_TBps": round(NOISE_BYTES_PER_GAUSSIAN * N / (med("noise_launch_ms") * 1e-3) / 1e12, 3),
            "hbm_launch_ms": med("noise_launch_rotating_ms"),
            "hbm_TBps": round(NOISE_BYTES_PER_GAUSSIAN * N / launch_s / 1e12, 3),
            "fraction_of_achievable_6.29_TBps": round(NOISE_BYTES_PER_GAUSSIAN * N / launch_s / 1e12 / HBM_ACHIEVABLE_TBPS, 3),
            "fused_vs_torch_rel_l2": [r["noise_fused_vs_torch_rel_l2"] for r in runs],
        },
        "relocation": {
            "drawn": {"fused_ms": med("relocate_fused_drawn_ms"), "torch_ms": med("relocate_torch_drawn_ms"),
                      "torch_over_fused": round(med("relocate_torch_drawn_ms") / med("relocate_fused_drawn_ms"), 2)},
            "pinned": {"fused_ms": med("relocate_fused_pinned_ms"), "torch_ms": med("relocate_torch_pinned_ms"),
                       "torch_over_fused": round(med("relocate_torch_pinned_ms") / med("relocate_fused_pinned_ms"), 2)},
        },
        "growth": {"fused_ms": med("add_fused_ms"), "torch_ms": med("add_torch_ms"),
                   "torch_over_fused": round(med("add_torch_ms") / med("add_fused_ms"), 2)},
    }
    text = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
