#!/usr/bin/env python
"""Cost of the normal-consistency loss at 1920x1080 and 1M Gaussians, each part against the same definitions in fp32
torch ops on the same GPU -- the route a user had before csrc/gsr_normals.hip.

    python tools/normal_bench.py --processes 3 --out profiles/normal_cost.json     # fresh child processes
    python tools/normal_bench.py --child                                           # one process, one JSON line
    python tools/normal_bench.py --ab-parent PARENT/libgsrast.so ...   # also bench.py cfg 3, parent against this build

* image kernel: `nc_fwd_launch_ms` / `nc_bwd_launch_ms` are the launches alone through ctypes, cycling over eight sets
  of planes (more than the 256 MiB Infinity Cache holds, so every launch reads from HBM): 24 and 44 B per pixel of
  compulsory traffic over that, against the 6.29 TB/s achievable HBM rate (the backward's halo re-reads are L2 hits and
  not counted).  `nc_fused_ms` is normal_consistency forward + E.mean().backward() under autograd, `nc_torch_ms` the same
  definition in torch ops (un-projection, central differences, cross product, normalisation, dot) under torch autograd.
  Device events around blocks of back-to-back calls, after warm-up; ms per call per block.
* geometry features: `geom_fwd_launch_ms` / `geom_bwd_launch_ms` likewise over eight sets of arrays (56 and 84 B per
  Gaussian); `geom_fused_ms` / `geom_torch_ms` forward + backward under autograd, fused against torch ops.
* --ab-parent: bench.py --config cfg3 --no-cpu-baseline --no-train-step in fresh processes, the parent build's library
  (through GSR_LIB) and this build's alternately; nothing cfg 3 runs is touched by this feature, so the expectation is
  that this build's median lies inside the parent's own run-to-run range.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_ACHIEVABLE_TBPS = 6.29
BYTES = dict(nc_fwd=24, nc_bwd=44, geom_fwd=56, geom_bwd=84)  # per pixel / per Gaussian, compulsory
ROTATE = 8


def torch_geometry(means, scales, rots, vm, torch):
    P = means.shape[0]
    q = rots / rots.norm(dim=1, keepdim=True)
    r, x, y, z = q.unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(P, 3, 3)
    k = scales.argmin(dim=1)
    n_v = R.gather(2, k.view(P, 1, 1).expand(P, 3, 1)).squeeze(2) @ vm[:3, :3]
    p_view = means @ vm[:3, :3] + vm[3, :3]
    flip = (n_v * p_view).sum(1, keepdim=True) > 0
    return torch.cat([torch.where(flip, -n_v, n_v), p_view[:, 2:3]], 1)


def torch_consistency(D, A, N, tanfovx, tanfovy, torch):
    _, H, W = D.shape
    live = A > 0
    d = torch.where(live, D / torch.where(live, A, torch.ones_like(A)), torch.zeros_like(D))[0]
    rx = (torch.arange(W, device=D.device, dtype=D.dtype) + 0.5 - W / 2) * (2 * tanfovx / W)
    ry = (torch.arange(H, device=D.device, dtype=D.dtype) + 0.5 - H / 2) * (2 * tanfovy / H)
    Pt = torch.stack([d * rx[None, :], d * ry[:, None], d])
    c = torch.linalg.cross(Pt[:, 2:, 1:-1] - Pt[:, :-2, 1:-1], Pt[:, 1:-1, 2:] - Pt[:, 1:-1, :-2], dim=0)
    sq = (c * c).sum(0, keepdim=True)
    ok = sq > 0
    unit = torch.where(ok, c * torch.rsqrt(torch.where(ok, sq, torch.ones_like(sq))), torch.zeros_like(c))
    n_d = torch.nn.functional.pad(unit, (1, 1, 1, 1))
    return 1 - A.detach() * (N * n_d).sum(0, keepdim=True)


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


def child(H, W, P):
    import torch
    from gaussian_splatting_lightning_amd import (GaussianRasterizationSettings, _native, geometry_features,
                                                  normal_consistency)
    from gaussian_splatting_lightning_amd.synthetic import TREEHILL_V0
    assert torch.cuda.is_available(), "normal_bench needs a HIP device: there is no CPU path to time"
    lib = _native.load()
    stream = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(0)
    tx, ty = 0.6, 0.6 * H / W
    out = {"H": H, "W": W, "P": P}
    rand = lambda *s: torch.rand(*s, device="cuda", generator=g)  # noqa: E731
    randn = lambda *s: torch.randn(*s, device="cuda", generator=g)  # noqa: E731
    turn = [0]

    def rotating(call):
        def fn():
            i = turn[0] % ROTATE
            turn[0] += 1
            call(i)
        return fn

    ptr = lambda ts: [t.data_ptr() for t in ts]  # noqa: E731
    planes = []
    for _ in range(ROTATE):
        A = 0.2 + 0.8 * rand(1, H, W)
        planes.append((A * (3 + 2 * rand(1, H, W)), A, randn(3, H, W)))
    dE = randn(1, H, W)
    E = torch.empty(1, H, W, device="cuda")
    grads = (torch.empty(1, H, W, device="cuda"), torch.empty(1, H, W, device="cuda"), torch.empty(3, H, W, device="cuda"))
    out["nc_fwd_launch_ms"] = blocks(rotating(lambda i: lib.gsr_normal_consistency_forward(
        H, W, tx, ty, *ptr(planes[i]), E.data_ptr(), None, stream)), torch, 500, warmup=50)
    out["nc_bwd_launch_ms"] = blocks(rotating(lambda i: lib.gsr_normal_consistency_backward(
        H, W, tx, ty, *ptr(planes[i]), dE.data_ptr(), *ptr(grads), stream)), torch, 500, warmup=50)
    rs = GaussianRasterizationSettings(H, W, tx, ty, None, 1.0, None, None, 0, None, False, False, False)

    def image_step(fn):
        leaves = [t.detach().requires_grad_(True) for t in planes[0]]
        fn(*leaves).mean().backward()
        return leaves

    fused = lambda D, A, N: normal_consistency(D, A, N, rs)  # noqa: E731
    plain = lambda D, A, N: torch_consistency(D, A, N, tx, ty, torch)  # noqa: E731
    out["nc_fused_ms"] = blocks(lambda: image_step(fused), torch, 50)
    out["nc_torch_ms"] = blocks(lambda: image_step(plain), torch, 20, warmup=5)
    x, y = image_step(fused), image_step(plain)
    out["nc_grad_vs_torch_rel_l2"] = [float((p.grad - r.grad).double().norm() / r.grad.double().norm())
                                      for p, r in zip(x, y)]

    vm = torch.tensor(TREEHILL_V0, device="cuda")
    sets = [(randn(P, 3), torch.exp(randn(P, 3) * 0.7 - 3), randn(P, 4)) for _ in range(ROTATE)]
    feat, up = torch.empty(P, 4, device="cuda"), randn(P, 4)
    dm, dq = torch.empty(P, 3, device="cuda"), torch.empty(P, 4, device="cuda")
    out["geom_fwd_launch_ms"] = blocks(rotating(lambda i: lib.gsr_geomfeat_forward(
        P, *ptr(sets[i]), vm.data_ptr(), feat.data_ptr(), stream)), torch, 1000, warmup=100)
    out["geom_bwd_launch_ms"] = blocks(rotating(lambda i: lib.gsr_geomfeat_backward(
        P, *ptr(sets[i]), vm.data_ptr(), up.data_ptr(), dm.data_ptr(), dq.data_ptr(), stream)), torch, 1000, warmup=100)

    def geom_step(fn):
        leaves = [t.detach().requires_grad_(True) for t in sets[0]]
        fn(*leaves).backward(up)
        return leaves

    out["geom_fused_ms"] = blocks(lambda: geom_step(lambda m, s, q: geometry_features(m, s, q, vm)), torch, 50)
    out["geom_torch_ms"] = blocks(lambda: geom_step(lambda m, s, q: torch_geometry(m, s, q, vm, torch)), torch, 20)
    x = geom_step(lambda m, s, q: geometry_features(m, s, q, vm))
    y = geom_step(lambda m, s, q: torch_geometry(m, s, q, vm, torch))
    out["geom_grad_vs_torch_rel_l2"] = [float((x[i].grad - y[i].grad).double().norm() / y[i].grad.double().norm())
                                        for i in (0, 2)]
    print(json.dumps(out))


def summarise(runs):
    res = {}
    for k in [k for k in runs[0] if k.endswith("_ms")]:
        per_process = [statistics.median(r[k]) for r in runs]
        res[k] = dict(samples=[[round(x, 5) for x in r[k]] for r in runs],
                      process_medians=[round(x, 5) for x in per_process], median=round(statistics.median(per_process), 5),
                      min=round(min(per_process), 5), max=round(max(per_process), 5))
    return res


def headline(parent_lib, rounds, steps, warmup, timeout):
    """bench.py cfg 3 in fresh processes, the parent's library and this build's alternately; ms per step."""
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
           str(warmup), "--config", "cfg3", "--no-cpu-baseline", "--no-train-step"]
    times = {"parent": [], "change": []}
    for _ in range(rounds):
        for which in ("parent", "change"):
            env = dict(os.environ)
            if which == "parent":
                env["GSR_LIB"] = os.path.abspath(parent_lib)
            else:
                env.pop("GSR_LIB", None)
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env, cwd=REPO)
            if r.returncode != 0:
                sys.exit(f"bench.py failed ({r.returncode}) with the {which} library, nothing further is started:\n"
                         f"{r.stdout}\n{r.stderr}")
            times[which].append(json.loads(r.stdout.strip().splitlines()[-1])["ms_per_step"])
    p, c = times["parent"], times["change"]
    return {"method": " ".join(cmd[1:]).replace(REPO + os.sep, "") + f": the parent commit's library and this change's "
            f"alternately in one session, {rounds} fresh processes each; ms per step",
            "parent_ms_per_step": p, "change_ms_per_step": c, "parent_min": min(p), "parent_max": max(p),
            "parent_median": statistics.median(p), "change_median": statistics.median(c),
            "change_median_inside_parent_range": min(p) <= statistics.median(c) <= max(p)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--H", type=int, default=1080)
    ap.add_argument("--W", type=int, default=1920)
    ap.add_argument("--P", type=int, default=1_000_000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--ab-parent", default=None, help="the parent build's libgsrast.so: also the bench.py cfg 3 A/B")
    ap.add_argument("--ab-rounds", type=int, default=5)
    ap.add_argument("--ab-steps", type=int, default=100)
    ap.add_argument("--ab-warmup", type=int, default=20)
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds each child process may take")
    a = ap.parse_args()
    if a.child:
        child(a.H, a.W, a.P)
        return
    runs = []
    for _ in range(a.processes):  # this process never opens the GPU: every child starts fresh
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--H", str(a.H), "--W", str(a.W),
                            "--P", str(a.P)], capture_output=True, text=True, timeout=a.timeout)
        if r.returncode != 0:
            sys.exit(f"a child process failed ({r.returncode}), nothing further is started:\n{r.stdout}\n{r.stderr}")
        runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    res = summarise(runs)
    med = lambda k: res[k]["median"]  # noqa: E731
    count = dict(nc_fwd=a.H * a.W, nc_bwd=a.H * a.W, geom_fwd=a.P, geom_bwd=a.P)
    tbps = lambda k: round(BYTES[k] * count[k] / (med(f"{k}_launch_ms") * 1e-3) / 1e12, 3)  # noqa: E731
    out = {
        "method": __doc__.split("\n\n", 2)[2].strip(),
        "workload": f"{a.W}x{a.H}, {a.P} Gaussians; {a.processes} fresh processes, medians of the process medians",
        "times": res,
        "consistency": {
            "fused_fwd_bwd_ms": med("nc_fused_ms"), "torch_fwd_bwd_ms": med("nc_torch_ms"),
            "torch_over_fused": round(med("nc_torch_ms") / med("nc_fused_ms"), 2),
            "fwd_launch_ms": med("nc_fwd_launch_ms"), "bwd_launch_ms": med("nc_bwd_launch_ms"),
            "grad_vs_torch_rel_l2": runs[0]["nc_grad_vs_torch_rel_l2"],
        },
        "geometry_features": {
            "fused_fwd_bwd_ms": med("geom_fused_ms"), "torch_fwd_bwd_ms": med("geom_torch_ms"),
            "torch_over_fused": round(med("geom_torch_ms") / med("geom_fused_ms"), 2),
            "fwd_launch_ms": med("geom_fwd_launch_ms"), "bwd_launch_ms": med("geom_bwd_launch_ms"),
            "grad_vs_torch_rel_l2": runs[0]["geom_grad_vs_torch_rel_l2"],
        },
        "bytes_per_element": BYTES,
        "hbm_TBps": {k: tbps(k) for k in BYTES},
        "fraction_of_achievable_6.29_TBps": {k: round(tbps(k) / HBM_ACHIEVABLE_TBPS, 3) for k in BYTES},
    }
    if a.ab_parent:
        out["headline"] = headline(a.ab_parent, a.ab_rounds, a.ab_steps, a.ab_warmup, a.timeout)
    text = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
