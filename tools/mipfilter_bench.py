#!/usr/bin/env python
"""Cost of Mip-Splatting's 3D smoothing filter at bench.py's cfg 3 count (1M Gaussians), each part against the same
definitions in fp32 torch ops on the same GPU -- the route a user had before csrc/gsr_mipfilter.hip.

    python tools/mipfilter_bench.py --processes 3 --out profiles/mipfilter_cost.json     # fresh child processes
    python tools/mipfilter_bench.py --child                                              # one process, one JSON line
    python tools/mipfilter_bench.py --bench-json FILE ...        # merges a record of bench.py figures as "headline"

* sampling rate, V = 200 look-at cameras on a ring (three focals), points 1.5 N(0, I): `rate_fused_ms` is
  mipfilter.sampling_rate (camera table built from device tensors, then the launch), `rate_launch_ms` the launch alone
  through ctypes, `rate_torch_ms` the per-camera Python loop of elementwise torch ops Mip-Splatting's trainer runs
  (view transform, three comparisons, running max / min / count).  Device events around blocks of back-to-back calls,
  after warm-up; ms per call per block.  The launch is VALU-bound: its issue fraction prices the wave-instructions of
  the ISA (13 per pair for the test, 4 of them packed; 17 more, one transcendental, in waves with a visible lane -- here
  counted for every wave, an upper bound on the work) with DESIGN.md's measured issue-rate model.
* filtered activations: `act_fused_ms` is FilteredGaussianActivations forward + backward under autograd,
  `act_torch_ms` the elementwise formulas (ratio form) under torch autograd; `act_fwd_launch_ms` / `act_bwd_launch_ms`
  are the launches alone cycling over six sets of arrays (more than the 256 MiB Infinity Cache holds, so every launch
  reads from HBM): 68 and 100 B per Gaussian over that, against the 6.29 TB/s achievable HBM rate.  The plain
  activations' launches (64 and 112 B) are timed the same way beside them.
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

HBM_ACHIEVABLE_TBPS = 6.29
BYTES = dict(act_fwd=68, act_bwd=100, plain_fwd=64, plain_bwd=112)
# DESIGN.md section 4, the issue-rate model: ns per wave-instruction per SIMD
NS_VALU, NS_PACKED, NS_TRANS, SIMDS = 1.29, 2.27, 3.5, 256 * 4
TEST_NS = 9 * NS_VALU + 4 * NS_PACKED           # per (wave, camera): the three dot products and comparisons
VISIBLE_NS = 16 * NS_VALU + 1 * NS_TRANS        # more in a wave with a visible lane: the division, max, min, count
ROTATE = 6


def cameras(V, torch):
    vm, tx, ty, w, h = [], [], [], [], []
    kinds = ((0.6, 0.4, 1920, 1280), (0.35, 0.5, 401, 573), (0.8, 0.3, 640, 240))
    for k in range(V):
        a = 0.1 + 2.0 * math.pi * k / V
        eye = torch.tensor([3.0 * math.cos(a), 0.5 * math.cos(2 * a), 3.0 * math.sin(a)], dtype=torch.float64)
        fwd = -eye / eye.norm()
        right = torch.linalg.cross(torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64), fwd)
        right = right / right.norm()
        up = torch.linalg.cross(fwd, right)
        m = torch.eye(4, dtype=torch.float64)
        m[:3, 0], m[:3, 1], m[:3, 2] = right, up, fwd
        m[3, :3] = -eye @ m[:3, :3]
        vm.append(m)
        t = kinds[k % 3]
        tx.append(t[0]); ty.append(t[1]); w.append(t[2]); h.append(t[3])
    f32 = dict(dtype=torch.float32, device="cuda")
    return dict(viewmatrix=torch.stack(vm).to(**f32), tanfovx=torch.tensor(tx, **f32), tanfovy=torch.tensor(ty, **f32),
                width=torch.tensor(w, **f32), height=torch.tensor(h, **f32))


def torch_sampling_rate(means, cams, torch, near=0.2, margin=0.15):
    """The per-camera loop, as Mip-Splatting's compute_3D_filter runs it."""
    P = means.shape[0]
    rate = torch.zeros(P, device=means.device)
    zmin = torch.full((P,), float("inf"), device=means.device)
    seen = torch.zeros(P, dtype=torch.int32, device=means.device)
    band = 1 + 2 * margin
    for k in range(cams["viewmatrix"].shape[0]):
        V = cams["viewmatrix"][k]
        pv = means @ V[:3, :3] + V[3, :3]
        x, y, z = pv[:, 0], pv[:, 1], pv[:, 2]
        vis = (z > near) & (x.abs() <= band * cams["tanfovx"][k] * z) & (y.abs() <= band * cams["tanfovy"][k] * z)
        fx = cams["width"][k] / (2 * cams["tanfovx"][k])
        rate = torch.where(vis, torch.maximum(rate, fx / z), rate)
        zmin = torch.where(vis, torch.minimum(zmin, z), zmin)
        seen = seen + vis.to(torch.int32)
    return rate, zmin, seen


def torch_activations(a, b, q, f, torch):
    s = torch.exp(a)
    sf = torch.sqrt(s * s + f * f)
    return sf, torch.sigmoid(b) * (s / sf).prod(1, keepdim=True), torch.nn.functional.normalize(q)


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


def child(N, V):
    import torch
    from gaussian_splatting_lightning_amd import _native
    from gaussian_splatting_lightning_amd.activations import GaussianActivations
    from gaussian_splatting_lightning_amd.mipfilter import (FilteredGaussianActivations, camera_table,
                                                            compute_3d_filter, sampling_rate)
    assert torch.cuda.is_available(), "mipfilter_bench needs a HIP device: there is no CPU path to time"
    lib = _native.load()
    stream = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(0)
    out = {"N": N, "V": V}

    means = 1.5 * torch.randn(N, 3, device="cuda", generator=g)
    cams = cameras(V, torch)
    table, _ = camera_table(cams, 0.15, "cuda")
    rate, zmin, seen = (torch.empty(N, device="cuda"), torch.empty(N, device="cuda"),
                        torch.empty(N, dtype=torch.int32, device="cuda"))

    def launch():
        lib.gsr_mipfilter_rate(N, means.data_ptr(), V, table.data_ptr(), 0.2, rate.data_ptr(), zmin.data_ptr(),
                               seen.data_ptr(), stream)

    out["rate_fused_ms"] = blocks(lambda: sampling_rate(means, cams), torch, 20, warmup=5)
    out["rate_launch_ms"] = blocks(launch, torch, 50, warmup=10)
    out["rate_torch_ms"] = blocks(lambda: torch_sampling_rate(means, cams, torch), torch, 2, nblocks=3, warmup=1)
    a, b = sampling_rate(means, cams), torch_sampling_rate(means, cams, torch)
    out["visible_pair_fraction"] = float(a[2].sum()) / (N * V)
    out["rate_seen_mismatches_vs_torch"] = int((a[2] != b[2]).sum())  # fp32 against fp32: pairs on a threshold may flip
    agree = (a[2] == b[2]) & (a[2] > 0)
    out["rate_vs_torch_max_rel"] = float(((a[0] - b[0]).abs() / b[0])[agree].max())

    sets = []
    for i in range(ROTATE):
        s = torch.randn(N, 3, device="cuda", generator=g) * 1.5 - 4.5
        o = torch.randn(N, 1, device="cuda", generator=g) * 2.0
        q = torch.randn(N, 4, device="cuda", generator=g)
        sets.append((s, o, q))
    f = compute_3d_filter(means, cams)
    ups = (torch.randn(N, 3, device="cuda", generator=g), torch.randn(N, 1, device="cuda", generator=g),
           torch.randn(N, 4, device="cuda", generator=g))
    outs = [tuple(torch.empty_like(t) for t in sets[0]) for _ in range(ROTATE)]
    ptr = lambda ts: [t.data_ptr() for t in ts]  # noqa: E731
    turn = [0]

    def rotating(call):
        def fn():
            i = turn[0] % ROTATE
            turn[0] += 1
            call(i)
        return fn

    launches = dict(
        act_fwd=lambda i: lib.gsr_activations_filter3d_forward(N, *ptr(sets[i]), f.data_ptr(), *ptr(outs[i]), stream),
        act_bwd=lambda i: lib.gsr_activations_filter3d_backward(N, *ptr(sets[i]), f.data_ptr(), *ptr(ups), *ptr(outs[i]),
                                                                stream),
        plain_fwd=lambda i: lib.gsr_activations_forward(N, *ptr(sets[i]), *ptr(outs[i]), stream),
        # the plain backward reads the raw rotation and the three activated tensors; any arrays of those shapes time it
        plain_bwd=lambda i: lib.gsr_activations_backward(N, sets[i][2].data_ptr(), *ptr(sets[i]), *ptr(ups),
                                                         *ptr(outs[i]), stream))
    for name, call in launches.items():
        out[f"{name}_launch_ms"] = blocks(rotating(call), torch, 2000, warmup=100)

    def step(activate):
        leaves = [t.detach().requires_grad_(True) for t in sets[0]]
        torch.autograd.backward(activate(*leaves), ups)
        return leaves

    out["act_fused_ms"] = blocks(lambda: step(lambda *t: FilteredGaussianActivations.apply(*t, f)), torch, 50)
    out["act_torch_ms"] = blocks(lambda: step(lambda *t: torch_activations(*t, f, torch)), torch, 50)
    out["plain_fused_ms"] = blocks(lambda: step(GaussianActivations.apply), torch, 50)
    x = step(lambda *t: FilteredGaussianActivations.apply(*t, f))
    y = step(lambda *t: torch_activations(*t, f, torch))
    out["act_grad_vs_torch_rel_l2"] = [float((p.grad - r.grad).double().norm() / r.grad.double().norm())
                                       for p, r in zip(x, y)]
    print(json.dumps(out))


def summarise(runs):
    res = {}
    for k in [k for k in runs[0] if k.endswith("_ms")]:
        per_process = [statistics.median(r[k]) for r in runs]
        res[k] = dict(samples=[[round(x, 5) for x in r[k]] for r in runs],
                      process_medians=[round(x, 5) for x in per_process], median=round(statistics.median(per_process), 5),
                      min=round(min(per_process), 5), max=round(max(per_process), 5))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--N", type=int, default=1_000_000)
    ap.add_argument("--V", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--bench-json", default=None, help="a JSON record of bench.py figures, merged in as 'headline'")
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds each child process may take")
    a = ap.parse_args()
    if a.child:
        child(a.N, a.V)
        return
    runs = []
    for _ in range(a.processes):  # this process never opens the GPU: every child starts fresh
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--N", str(a.N), "--V", str(a.V)],
                           capture_output=True, text=True, timeout=a.timeout)
        if r.returncode != 0:
            sys.exit(f"a child process failed ({r.returncode}), nothing further is started:\n{r.stdout}\n{r.stderr}")
        runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    res = summarise(runs)
    med = lambda k: res[k]["median"]  # noqa: E731
    N, V = a.N, a.V
    waves = math.ceil(N / 64)
    launch_s = med("rate_launch_ms") * 1e-3
    issue_s = waves * V * (TEST_NS + VISIBLE_NS) * 1e-9 / SIMDS
    tbps = lambda name: round(BYTES[name] * N / (med(f"{name}_launch_ms") * 1e-3) / 1e12, 3)  # noqa: E731
    out = {
        "method": __doc__.split("\n\n", 2)[2].strip(),
        "workload": f"{N} Gaussians, {V} cameras; {a.processes} fresh processes, medians of the process medians",
        "times": res,
        "sampling_rate": {
            "fused_call_ms": med("rate_fused_ms"), "launch_ms": med("rate_launch_ms"), "torch_loop_ms": med("rate_torch_ms"),
            "torch_over_fused": round(med("rate_torch_ms") / med("rate_fused_ms"), 1),
            "pairs_per_s": round(N * V / launch_s, 0),
            "valu_wave_instructions_per_pair": {"test": 13, "test_packed": 4, "visible_more": 17,
                                                "visible_transcendental": 1},
            "priced_issue_ms_all_waves_visible": round(issue_s * 1e3, 4),
            "issue_fraction_upper": round(issue_s / launch_s, 3),
            "issue_fraction_test_only": round(waves * V * TEST_NS * 1e-9 / SIMDS / launch_s, 3),
            "visible_pair_fraction": runs[0]["visible_pair_fraction"],
            "seen_mismatches_vs_fp32_torch": runs[0]["rate_seen_mismatches_vs_torch"],
            "rate_vs_torch_max_rel": runs[0]["rate_vs_torch_max_rel"],
        },
        "activations": {
            "fused_fwd_bwd_ms": med("act_fused_ms"), "torch_fwd_bwd_ms": med("act_torch_ms"),
            "torch_over_fused": round(med("act_torch_ms") / med("act_fused_ms"), 2),
            "plain_fused_fwd_bwd_ms": med("plain_fused_ms"),
            "bytes_per_gaussian": BYTES,
            "hbm_TBps": {k: tbps(k) for k in BYTES},
            "fraction_of_achievable_6.29_TBps": {k: round(tbps(k) / HBM_ACHIEVABLE_TBPS, 3) for k in BYTES},
            "grad_vs_torch_rel_l2": runs[0]["act_grad_vs_torch_rel_l2"],
        },
    }
    if a.bench_json:
        with open(a.bench_json) as fh:
            out["headline"] = json.load(fh)
    text = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
