#!/usr/bin/env python
"""Cost of the median depth map on bench.py's cfg 3 scene (1M Gaussians, 1920x1080, SH degree 3), beside the nearest
existing thing, the distortion map's walks, in the same run.

    python tools/median_bench.py --processes 3 --out profiles/median_cost.json     # fresh child processes
    python tools/median_bench.py --child                                           # one process, one JSON line
    python tools/median_bench.py --ab-parent PARENT/libgsrast.so ...   # also bench.py cfg 3, parent against this build

* One training-shaped step per iteration: forward_raw(..., return_alpha=True, distortion="z", median_depth=True) and
  backward_raw with the colour, inverse-depth, distortion and median upstream gradients, so the colour composite, the
  distortion walks and the median walks all run on the same recorded state.  The library's per-stage device events
  (gsr_set_profiling) bracket each launch: `median_fwd`, `median_bwd`, `distortion_fwd`, `distortion_bwd`, and for
  scale `render_fwd`, `render_bwd`; ms per launch, averaged over the profiled steps of a process after warm-up.
* `step_ms` / `step_plain_ms`: a host clock around blocks of such steps ending in a synchronise, with the median and
  without it (no events), interleaved block by block: what asking for the median adds to a step.
* The early exit is DERIVED, not counted by the kernel: the host applies the kernel's exit rule (gsr_median.hip) to
  what the forward left.  A tile's list holds ceil(tile_last / 32) batches; the
  wave leaves after the first batch at whose end no pixel is unfinished, a pixel being unfinished while its
  transmittance exceeds 1/2 (it crosses in the batch of its median's position when its final transmittance is <= 1/2)
  and its contributors go on (n_contrib past the batch).  `batches_skipped_fraction` = 1 - walked / total over all tiles.
* --ab-parent: bench.py --config cfg3 --no-cpu-baseline --no-train-step in fresh processes, the parent build's library
  (through GSR_LIB) and this build's alternately (tools/normal_bench.py's headline); nothing cfg 3 runs is touched by
  this feature, so the expectation is that this build's median lies inside the parent's own run-to-run range.
"""
import argparse
import importlib.util
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

STAGES = ("median_fwd", "median_bwd", "distortion_fwd", "distortion_bwd", "render_fwd", "render_bwd")
BATCH = 32  # gsr_replay.h REPLAY_BATCH


def early_exit_census(torch, _native, st, pos, W, H):
    """(batches walked, batches in all) of the median forward over the tiles, from the recorded state."""
    P = st.radii.shape[0]
    lay = _native.state_layout(P, st.num_rendered, W, H)
    gx, gy = (W + 15) // 16, (H + 15) // 16

    def view(off, n):
        return st.image_buffer[off: off + 4 * n].view(torch.int32).long()

    tile_last = view(lay["img_tile_last"], gx * gy)
    n_contrib = view(lay["img_n_contrib"], W * H).reshape(H, W)
    off = lay["img_final_T"]
    final_T = st.image_buffer[off: off + 4 * W * H].view(torch.float32).reshape(H, W)
    crossed = final_T <= 0.5  # (T only falls along the walk)
    # the batch at whose end the pixel is finished: its median's when T crosses 1/2 there, else its last contributor's
    done = torch.where(crossed & (pos >= 0), pos.long() // BATCH, (n_contrib - 1).clamp(min=0) // BATCH)
    done = torch.minimum(done, (n_contrib - 1).clamp(min=0) // BATCH)
    pad = torch.zeros(gy * 16, gx * 16, dtype=torch.long, device=done.device)
    pad[:H, :W] = done
    per_tile = pad.reshape(gy, 16, gx, 16).amax(dim=(1, 3)).reshape(-1)
    total = (tile_last + BATCH - 1) // BATCH
    walked = torch.minimum(per_tile + 1, total)
    return int(walked.sum()), int(total.sum())


def child(steps, warmup, blocks):
    import torch
    from gaussian_splatting_lightning_amd import _native
    from gaussian_splatting_lightning_amd.rasterizer import (GaussianRasterizationSettings, backward_raw,
                                                             forward_raw)
    from gaussian_splatting_lightning_amd.synthetic import make_camera, make_scene, make_upstream
    assert torch.cuda.is_available(), "median_bench needs a HIP device: there is no CPU path to time"
    dev = torch.device("cuda", 0)
    n, W, H, deg = 1_000_000, 1920, 1080, 3  # bench.py CONFIGS["cfg3"], view 0 of 8
    sc = make_scene(n, sh_degree=deg, seed=0, stress_fraction=0.0).to(dev)
    c = make_camera(W, H, view_index=0, num_views=8).to(dev)
    dcolor, dinv = (t.to(dev) for t in make_upstream(W, H, seed=0))
    g = torch.Generator(device="cuda").manual_seed(1)
    g_dist = torch.randn(1, H, W, device=dev, generator=g)
    g_med = torch.randn(1, H, W, device=dev, generator=g)
    rs = GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=c.tanfovx, tanfovy=c.tanfovy, bg=torch.zeros(3, device=dev),
        scale_modifier=1.0, viewmatrix=c.viewmatrix, projmatrix=c.projmatrix, sh_degree=deg, campos=c.campos,
        prefiltered=False, debug=False, antialiasing=False)

    def step(median=True):
        res = forward_raw(sc.means3D, sc.shs, None, sc.opacities, sc.scales, sc.rotations, None, rs,
                          return_alpha=True, distortion="z", median_depth=median)
        kw = dict(grad_out_median_depth=g_med) if median else {}
        backward_raw(res[-1], rs, dcolor, dinv, grad_out_distortion=g_dist, **kw)
        return res

    for _ in range(warmup):
        step(True)
        step(False)
    torch.cuda.synchronize()
    _native.reset_stage_times()
    _native.set_profiling(True)
    for _ in range(steps):
        res = step(True)
    torch.cuda.synchronize()
    _native.set_profiling(False)
    times = _native.stage_times()
    out = {"steps": steps, **{f"{k}_ms": times[k][0] / max(times[k][1], 1) for k in STAGES},
           **{f"{k}_calls": times[k][1] for k in STAGES}}

    def block(median):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step(median)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / steps

    out["step_ms"], out["step_plain_ms"] = [], []
    for _ in range(blocks):
        out["step_ms"].append(block(True))
        out["step_plain_ms"].append(block(False))
    alpha, md, mi, st = res[3], res[-3], res[-2], res[-1]
    walked, total = early_exit_census(torch, _native, st, st.median.pos, W, H)
    out.update(batches_walked=walked, batches_total=total, num_rendered=st.num_rendered,
               pixels_reached=int((mi >= 0).sum()), pixels_half_opaque=int(((1.0 - alpha) <= 0.5).sum()),
               distinct_medians=int(torch.unique(mi).numel() - int(bool((mi < 0).any()))))
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--ab-parent", default=None, help="the parent build's libgsrast.so: also the bench.py cfg 3 A/B")
    ap.add_argument("--ab-rounds", type=int, default=5)
    ap.add_argument("--ab-steps", type=int, default=100)
    ap.add_argument("--ab-warmup", type=int, default=20)
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds each child process may take")
    a = ap.parse_args()
    if a.child:
        child(a.steps, a.warmup, a.blocks)
        return
    runs = []
    for _ in range(a.processes):  # this process never opens the GPU: every child starts fresh
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--steps", str(a.steps), "--warmup",
                            str(a.warmup), "--blocks", str(a.blocks)], capture_output=True, text=True,
                           timeout=a.timeout)
        if r.returncode != 0:
            sys.exit(f"a child process failed ({r.returncode}), nothing further is started:\n{r.stdout}\n{r.stderr}")
        runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    med = lambda k: round(statistics.median(statistics.median(r[k]) if isinstance(r[k], list) else r[k]  # noqa: E731
                                            for r in runs), 5)
    ms = {f"{k}_ms": dict(process_values=[round(r[f"{k}_ms"], 5) for r in runs], median=med(f"{k}_ms")) for k in STAGES}
    for k in ("step_ms", "step_plain_ms"):
        ms[k] = dict(process_values=[[round(x, 5) for x in r[k]] for r in runs], median=med(k))
    r0 = runs[0]
    out = {
        "method": __doc__.split("\n\n", 2)[2].strip(),
        "workload": f"bench.py cfg 3: 1000000 Gaussians, 1920x1080, SH degree 3, view 0 of 8; {a.processes} fresh "
                    f"processes of {a.steps} profiled steps, medians over the processes",
        "times": ms,
        "median_over_distortion": {
            "forward": round(med("median_fwd_ms") / med("distortion_fwd_ms"), 3),
            "backward": round(med("median_bwd_ms") / med("distortion_bwd_ms"), 3)},
        "median_over_colour_composite": {
            "forward": round(med("median_fwd_ms") / med("render_fwd_ms"), 3),
            "backward": round(med("median_bwd_ms") / med("render_bwd_ms"), 3)},
        "step_added_ms": round(med("step_ms") - med("step_plain_ms"), 5),
        "early_exit": {
            "batches_total": r0["batches_total"], "batches_walked": r0["batches_walked"],
            "batches_skipped_fraction": round(1.0 - r0["batches_walked"] / max(r0["batches_total"], 1), 4),
            "derived": "from final_T, n_contrib and median_pos by the kernel's exit rule restated on the host; the kernel "
                       "keeps no counter",
            "pixels_reached": r0["pixels_reached"], "pixels_half_opaque": r0["pixels_half_opaque"],
            "distinct_medians": r0["distinct_medians"], "num_rendered": r0["num_rendered"]},
    }
    if a.ab_parent:
        spec = importlib.util.spec_from_file_location("normal_bench", os.path.join(REPO, "tools", "normal_bench.py"))
        nb = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(nb)
        out["headline"] = nb.headline(a.ab_parent, a.ab_rounds, a.ab_steps, a.ab_warmup, a.timeout)
    text = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
