#!/usr/bin/env python
"""Bilateral-grid slice forward, slice backward and TV at 1920x1080 with a 16x16x8 grid and num = 200: hipEvent medians
of the fused kernels (csrc/gsr_bilagrid.hip) against the torch route on the same device -- the definition through
F.grid_sample on a 5-D tensor plus elementwise ops, as gsplat's lib_bilagrid does it.  Writes
profiles/bilagrid_cost.json (or --out).  --bench-json FILE merges a record of bench.py figures into the result under
"bench_cfg3_when_unused" (the rasterizer's path does not touch this code; the record shows it).

Algorithmic bytes: the forward reads and writes three planes (24 B/px); the backward reads the image and the upstream
gradient twice (once per kernel) and writes the image gradient (60 B/px) plus one memset of all num grids.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _blocks(fn, blocks, min_ms=50.0):
    """Median material: `blocks` hipEvent timings of back-to-back calls, each block sized to last at least `min_ms`
    (20 calls at the least), in ms per call."""
    import torch

    def timed(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / calls

    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    calls = max(20, min(5000, int(min_ms / max(timed(5), 1e-4)) + 1))
    return [round(timed(calls), 5) for _ in range(blocks)]


def torch_slice(grids, image, idx):
    import torch
    import torch.nn.functional as F
    B, _, H, W = image.shape
    x = (torch.arange(W, device=image.device, dtype=image.dtype) + 0.5) / W
    y = (torch.arange(H, device=image.device, dtype=image.dtype) + 0.5) / H
    gray = 0.299 * image[:, 0] + 0.587 * image[:, 1] + 0.114 * image[:, 2]
    coords = torch.stack([x.view(1, 1, W).expand(B, H, W), y.view(1, H, 1).expand(B, H, W), gray], dim=-1)
    A = F.grid_sample(grids[idx], ((coords - 0.5) * 2).unsqueeze(1), mode="bilinear", align_corners=True,
                      padding_mode="border")
    A = A[:, :, 0].reshape(B, 3, 4, H, W)
    return (A[:, :, :3] * image[:, None]).sum(2) + A[:, :, 3]


def torch_tv(grids):
    tv = 0.0
    for axis in (2, 3, 4):
        n = grids.shape[axis]
        if n > 1:
            tv = tv + grids.diff(dim=axis).pow(2).sum() / (grids[0].numel() // n * (n - 1))
    return tv / grids.shape[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles",
                                                  "bilagrid_cost.json"))
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--min-block-ms", type=float, default=50.0)
    ap.add_argument("--bench-json", default=None)
    a = ap.parse_args()
    import torch
    from gaussian_splatting_lightning_amd.bilagrid import BilateralGrid, slice_image, total_variation_loss
    dev = torch.device("cuda", 0)
    num, L, Gh, Gw, H, W = 200, 8, 16, 16, 1080, 1920
    g = torch.Generator().manual_seed(0)
    bg = BilateralGrid(num, Gw, Gh, L).to(dev)
    with torch.no_grad():
        bg.grids.add_(0.1 * torch.randn(bg.grids.shape, generator=g).to(dev))
    grids = bg.grids
    image = torch.rand(1, 3, H, W, generator=g).to(dev).requires_grad_(True)
    dout = torch.randn(1, 3, H, W, generator=g).to(dev)
    idx = [17]
    tidx = torch.tensor(idx, device=dev)

    def clear():
        grids.grad = image.grad = None

    res = {"workload": f"{W}x{H} image, {Gw}x{Gh}x{L} grid, num = {num}, fp32",
           "method": f"hipEvents around blocks of back-to-back calls lasting at least {a.min_block_ms} ms each, "
                     f"{a.blocks} blocks, median of the blocks; "
                     "backward = autograd backward of the slice alone under a fixed upstream gradient (gradients "
                     "to the grids and the image; the fused one includes the memset of all num grids, the torch "
                     "one the index_put of grids[idx]); tv = forward + backward of the total variation",
           "ms_per_call": {}}
    routes = {"fused": (lambda: slice_image(grids, image, idx), lambda: total_variation_loss(grids)),
              "torch": (lambda: torch_slice(grids, image, tidx), lambda: torch_tv(grids))}
    for name, (sl, tv) in routes.items():
        with torch.no_grad():
            fwd = _blocks(sl, a.blocks, a.min_block_ms)
        out = sl()

        def bwd():
            clear()
            out.backward(dout, retain_graph=True)

        def tv_both():
            clear()
            tv().backward()

        res["ms_per_call"][name] = {"slice_forward": fwd, "slice_backward": _blocks(bwd, a.blocks, a.min_block_ms),
                                    "tv_forward_backward": _blocks(tv_both, a.blocks, a.min_block_ms)}
        del out
        clear()
    # the fused backward's two halves, through the C entry point (a NULL output skips its kernels)
    import ctypes

    from gaussian_splatting_lightning_amd import _native
    lib = _native.load()
    gd, xd = grids.detach(), image.detach()
    dg, dx, c_idx = torch.empty_like(gd), torch.empty_like(xd), (ctypes.c_int32 * 1)(*idx)
    nbytes = lib.gsr_bilagrid_workspace_bytes(L, Gh, Gw, H, W)
    ws = torch.empty(max(nbytes // 4, 1), device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def half(dg_ptr, dx_ptr):
        _native.check(lib.gsr_bilagrid_slice_backward(num, L, Gh, Gw, gd.data_ptr(), 1, H, W, xd.data_ptr(), c_idx,
                                                      dout.data_ptr(), dg_ptr, dx_ptr, ws.data_ptr(), stream), "bench")

    res["ms_per_call"]["fused_backward_halves"] = {
        "grid_gradient_with_memset": _blocks(lambda: half(dg.data_ptr(), None), a.blocks, a.min_block_ms),
        "image_gradient": _blocks(lambda: half(None, dx.data_ptr()), a.blocks, a.min_block_ms)}
    res["grid_gradient_splits"] = nbytes // (gd[0].numel() * 4) if nbytes else 1
    med = {r: {k: statistics.median(v) for k, v in d.items()} for r, d in res["ms_per_call"].items()}
    res["median_ms_per_call"] = med
    res["torch_over_fused"] = {k: round(med["torch"][k] / med["fused"][k], 2) for k in med["fused"]}
    px = H * W
    res["fused_algorithmic_GBps"] = {
        "slice_forward": round(24 * px / (med["fused"]["slice_forward"] * 1e-3) / 1e9, 1),
        "slice_backward": round((60 * px + grids.numel() * 4) / (med["fused"]["slice_backward"] * 1e-3) / 1e9, 1)}
    # the two routes compute the same thing
    with torch.no_grad():
        d = (slice_image(grids, image, idx) - torch_slice(grids, image, tidx)).abs().max()
    res["max_abs_difference_fused_vs_torch"] = float(d)
    if a.bench_json:
        res["bench_cfg3_when_unused"] = json.load(open(a.bench_json))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"median_ms_per_call": med, "torch_over_fused": res["torch_over_fused"]}))


if __name__ == "__main__":
    main()
