#!/usr/bin/env python
"""What the depth distortion map costs: profiles/distortion_cost.json.

bench.py's scene and view of a config (cfg3 by default).  One forward_raw + backward_raw call (SH colour and inverse
depth gradients) is timed
    plain:      without distortion,
    z / ndc:    with the distortion map and its upstream gradient,
    features3:  with C = 3 feature channels (1, t, t^2) and their upstream gradient -- the call that renders the squared
                form 2 (A Q - M^2) today, the yardstick,
in alternating blocks (hipEvents around a block of calls, the median of the blocks), and the per-stage hipEvent times of
the distortion kernels in a separate pass.  (The record's `bench_cfg3_when_unused` section is not written here: it holds
bench.py runs of the parent commit's library and this one's, alternately, in the same session.)

Usage:  python profiles/distortion_cost.py [--config cfg3] [--blocks 5] [--calls 20] [--out profiles/distortion_cost.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench  # noqa: E402
from gaussian_splatting_lightning_amd import GaussianRasterizationSettings, _native  # noqa: E402
from gaussian_splatting_lightning_amd.rasterizer import backward_raw, forward_raw  # noqa: E402
from gaussian_splatting_lightning_amd.synthetic import make_camera, make_scene, make_upstream  # noqa: E402

NEAR, FAR = 0.2, 1000.0  # 2DGS's planes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg3", choices=sorted(bench.CONFIGS))
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "distortion_cost.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = bench.CONFIGS[args.config]
    n, W, H, deg = cfg["n"], cfg["W"], cfg["H"], cfg["deg"]
    sc = make_scene(n, sh_degree=deg, seed=0, stress_fraction=cfg["stress"]).to(dev)
    c = make_camera(W, H, view_index=0, num_views=8 if args.config == "cfg3" else 1).to(dev)
    dcolor, dinv = (t.to(dev) for t in make_upstream(W, H, seed=0))
    rs = GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=c.tanfovx, tanfovy=c.tanfovy, bg=torch.zeros(3, device=dev),
        scale_modifier=1.0, viewmatrix=c.viewmatrix, projmatrix=c.projmatrix, sh_degree=deg, campos=c.campos,
        prefiltered=False, debug=False, antialiasing=False)
    gen = torch.Generator(device="cpu").manual_seed(1)
    gD = torch.randn(1, H, W, generator=gen).to(dev)
    dF = torch.randn(3, H, W, generator=gen).to(dev)
    z = (sc.means3D @ c.viewmatrix[:3, 2] + c.viewmatrix[3, 2]).clamp_min(NEAR)
    t = FAR / (FAR - NEAR) * (1 - NEAR / z)
    feats = torch.stack([torch.ones_like(t), t, t * t], 1).contiguous()

    def call(kind):
        kw = {}
        if kind in ("z", "ndc"):
            kw = dict(distortion=kind, distortion_near=NEAR, distortion_far=FAR)
        elif kind == "features3":
            kw = dict(features=feats)
        res = forward_raw(sc.means3D, sc.shs, None, sc.opacities, sc.scales, sc.rotations, None, rs, **kw)
        bk = {}
        if kind in ("z", "ndc"):
            bk = dict(grad_out_distortion=gD)
        elif kind == "features3":
            bk = dict(grad_out_features=dF)
        backward_raw(res[-1], rs, dcolor, dinv, **bk)
        return res

    kinds = ("plain", "z", "ndc", "features3")
    for k in kinds:  # warm-up: allocator, first launches
        for _ in range(3):
            res = call(k)
    instances = int(res[-1].num_rendered)
    torch.cuda.synchronize()
    times = {k: [] for k in kinds}
    for _ in range(args.blocks):
        for k in kinds:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.calls):
                call(k)
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) / args.calls)
    med = {k: statistics.median(v) for k, v in times.items()}

    # per-stage events of the distortion kernels, in a pass of their own
    stages = {}
    _native.set_profiling(True)
    for k in ("z", "ndc", "features3"):
        _native.load().gsr_reset_stage_times()
        for _ in range(args.calls):
            call(k)
        torch.cuda.synchronize()
        st = _native.stage_times()
        stages[k] = {name: round(tot / args.calls, 5) for name, (tot, cnt) in st.items()
                     if cnt and name.startswith(("distortion_", "feat_"))}
    _native.set_profiling(False)

    out = dict(
        method=" ".join(__doc__.split("\n\n")[1].split()),
        config=args.config, instances=instances, blocks=args.blocks, calls_per_block=args.calls, planes=[NEAR, FAR],
        ms_per_call={k: [round(x, 5) for x in v] for k, v in times.items()},
        median_ms_per_call={k: round(v, 5) for k, v in med.items()},
        added_ms={k: round(med[k] - med["plain"], 5) for k in kinds if k != "plain"},
        added_fraction={k: round((med[k] - med["plain"]) / med["plain"], 4) for k in kinds if k != "plain"},
        stage_ms_per_call=stages,
        state_bytes_added=2 * 4 * W * H, map_bytes=4 * W * H, backward_scratch_bytes_added=0)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["median_ms_per_call"]), json.dumps(out["added_ms"]), json.dumps(stages))


if __name__ == "__main__":
    main()
