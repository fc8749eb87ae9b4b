"""The composites' walk bodies without the exponent-sign test (knob definite_fast) against the generic bodies, bit for
bit, on the GPU.

A batch of 64 staged instances runs the DEFINITE body when every one of them passes conic_is_definite (gsr_common.h),
else the generic body; both must make the same decisions, so every output is the same bits with definite_fast 1 and 0.
Scene: 128x128 (8x8 tiles), 4000 Gaussians of synthetic.make_scene plus 64 needles -- scales (3, 1e-3, 1e-3), random
rotations: tens to hundreds of pixels long and the reference's 0.3 px^2 dilation across, so their conics' eigenvalue
ratio is below the classifier's 1e-4 -- which span the image, so that most tiles' batches mix the two classes (and the
batches of the tiles they miss do not); opacities above 0.99 and below 1/255; and one Gaussian centred exactly on a
pixel centre, where the exponent is exactly 0.  The numpy classifier of tests/test_definite_conic_host.py, on the
forward state's records, asserts that mix.

Settings: the default launch at this size (4 part-waves per tile with checkpoints, the segmented backward), whole tiles
(with the strip masks), the 2-part forward with the 4-part backward, the union walk, and the alpha / background-image
call (the EXT forms) under the default launch and whole tiles."""
import functools

import numpy as np
import pytest
import torch

from tests.helpers import hip_state_arrays, run_hip, scene_inputs, settings_for, upstream
from tests.test_definite_conic_host import conic_is_definite

pytestmark = pytest.mark.gpu

N, NEEDLES, W, H, SEED = 4000, 64, 128, 128, 21
HIGH, LOW = slice(0, 150), slice(150, 300)  # Gaussians given opacities above 0.99 / around and below 1/255
f32 = np.float32


def _xy_of(means, base, dev):
    """Screen positions the preprocess gives to Gaussians at `means` (tiny, isotropic), from the forward state."""
    n = len(means)
    inp = dict(base, means3D=np.ascontiguousarray(means, f32), opacities=np.full((n, 1), 0.5, f32),
               scales=np.full((n, 3), 1e-3, f32), rotations=np.tile(np.asarray([1, 0, 0, 0], f32), (n, 1)),
               shs=np.zeros((n,) + base["shs"].shape[1:], f32))
    out = run_hip(inp, dev)
    assert (out["radii"] > 0).all()
    return hip_state_arrays(out)["xy"].astype(np.float64)


@functools.lru_cache(maxsize=None)
def _on_centre_mean(dev):
    """A world position the preprocess projects exactly onto a pixel centre (integer coordinates in fp32), near the
    world origin where the fp32 steps of the mean are ~1e-9 (1e-7 px; a pixel coordinate near 64 steps by 7.6e-6): a
    few Newton steps on the preprocess's own output, then a 128 x 128 grid of neighbours, one forward."""
    base = scene_inputs(4, W, H, sh_degree=1, seed=SEED)
    m = np.zeros(3)
    target = np.rint(_xy_of(m[None], base, dev)[0])
    d = 1e-3
    for _ in range(4):
        xy = _xy_of(np.stack([m, m + [d, 0, 0], m + [0, d, 0]]), base, dev)
        J = np.stack([(xy[1] - xy[0]) / d, (xy[2] - xy[0]) / d], 1)
        m[:2] += np.linalg.solve(J, target - xy[0])
    i, j = np.meshgrid(np.arange(-64, 64), np.arange(-64, 64), indexing="ij")
    cand = np.tile(m, (i.size, 1))
    cand[:, 0] += 1.5e-8 * i.reshape(-1)
    cand[:, 1] += 1.5e-8 * j.reshape(-1)
    cand = cand.astype(f32)
    xy = _xy_of(cand, base, dev)
    hit = np.flatnonzero((xy == target).all(1))
    assert len(hit), "no fp32 position near the origin projects exactly onto the pixel centre"
    return cand[hit[len(hit) // 2]], target


@functools.lru_cache(maxsize=None)
def _scene(dev):
    """(inputs, dL_dcolor, dL_dinvdepth, dL_dalpha, background image, index of the on-centre Gaussian, its pixel)."""
    inp = scene_inputs(N, W, H, sh_degree=1, seed=SEED)
    rng = np.random.default_rng(SEED)
    centre, pixel = _on_centre_mean(dev)
    k = NEEDLES + 1
    means = np.concatenate([inp["means3D"], (0.4 * rng.standard_normal((NEEDLES, 3))).astype(f32), centre[None]])
    scales = np.concatenate([inp["scales"], np.tile(np.asarray([3.0, 1e-3, 1e-3], f32), (NEEDLES, 1)),
                             np.full((1, 3), 0.03, f32)])
    q = rng.standard_normal((k, 4))
    rots = np.concatenate([inp["rotations"], (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(f32)])
    opac = np.concatenate([inp["opacities"], rng.uniform(0.2, 0.7, (NEEDLES, 1)).astype(f32), np.full((1, 1), 0.8, f32)])
    opac[HIGH] = rng.uniform(0.99, 1.0, (150, 1)).astype(f32)
    opac[HIGH.start] = 1.0
    opac[LOW] = rng.uniform(0.0, 2.0 / 255.0, (150, 1)).astype(f32)  # both sides of 1/255
    shs = np.concatenate([inp["shs"], (0.3 * rng.standard_normal((k,) + inp["shs"].shape[1:])).astype(f32)])
    inp = dict(inp, means3D=means, scales=scales, rotations=rots, opacities=opac, shs=shs)
    dc, di = upstream(W, H, SEED)
    return inp, dc, di, rng.standard_normal((1, H, W)).astype(f32), rng.random((3, H, W), dtype=f32), N + NEEDLES, pixel


def _t(a, dev):
    return None if a is None else torch.as_tensor(np.asarray(a, f32), device=dev)


def _bits(t):
    """Bit patterns (a NaN compares by its bits, and -0 differs from 0)."""
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _strip_masks(st, hs):
    """The forward's per-instance strip masks (BinningState::strip_mask: R bytes in the binning buffer, the 256-B
    aligned block after inv) at the instances it loaded."""
    from gaussian_splatting_lightning_amd import _native
    R = st.num_rendered
    lay = _native.state_layout(st.means3D.shape[0], R, W, H)
    off = (lay["bin_inv"] + 4 * R + 255) // 256 * 256
    sm = st.binning_buffer[off: off + R].cpu().numpy()
    loaded = np.zeros(R, bool)
    for (r0, _), n in zip(hs["ranges"], hs["tile_loaded"]):
        loaded[int(r0): int(r0) + int(n)] = True
    return sm[loaded]


def _render(dev, ext, whole):
    """Forward and backward of the scene; every output and state array the two knob values must agree on."""
    from gaussian_splatting_lightning_amd.rasterizer import backward_raw, forward_raw
    inp, dc, di, da, image, _, _ = _scene(dev)
    rs = settings_for(inp, dev)
    if ext:
        rs = rs._replace(bg=_t(image, dev))
    res = forward_raw(_t(inp["means3D"], dev), _t(inp["shs"], dev), None, _t(inp["opacities"], dev),
                      _t(inp["scales"], dev), _t(inp["rotations"], dev), None, rs, return_alpha=ext)
    color, radii, invd, st = res[0], res[1], res[2], res[-1]
    out = dict(color=color, radii=radii, invdepth=invd)
    if ext:
        out["alpha"] = res[3]
    hs = hip_state_arrays(dict(state=st, color=color.cpu().numpy(), radii=radii.cpu().numpy()))
    out.update(final_T=hs["final_T"], n_contrib=hs["n_contrib"], tile_last=hs["tile_last"],
               tile_loaded=hs["tile_loaded"], point_list=hs["point_list_written"])
    if whole:
        out["strip_mask"] = _strip_masks(st, hs)
    g = backward_raw(st, rs, _t(dc, dev), _t(di, dev), grad_out_alpha=_t(da, dev) if ext else None,
                     background_grad=ext)
    for k, v in g.items():
        if torch.is_tensor(v):
            out["grad_" + k] = v
    torch.cuda.synchronize()
    return {k: _bits(v) for k, v in out.items()}, hs


def test_scene_mixes_the_two_classes(gpu_device):
    from gaussian_splatting_lightning_amd import _native
    inp, _, _, _, _, centre, pixel = _scene(gpu_device)
    with _native.tuned(definite_fast=0):
        out = run_hip(inp, gpu_device)
    hs = hip_state_arrays(out)
    gx = (W + 15) // 16
    tile_of, gid = [], []
    for t, ((r0, _), n) in enumerate(zip(hs["ranges"], hs["tile_loaded"])):
        tile_of.append(np.full(int(n), t))
        gid.append(hs["point_list_written"][int(r0): int(r0) + int(n)].astype(np.int64))
    tile_of, gid = np.concatenate(tile_of), np.concatenate(gid)
    xy, co = hs["xy"][gid], hs["conic_opacity"][gid]
    definite = conic_is_definite(xy[:, 0], xy[:, 1], co[:, 0], co[:, 1], co[:, 2], co[:, 3],
                                 (tile_of % gx * 16).astype(f32), (tile_of // gx * 16).astype(f32))
    n_def = np.bincount(tile_of, definite, gx * gx)
    n_gen = np.bincount(tile_of, ~definite, gx * gx)
    mixed = int(((n_def > 0) & (n_gen > 0)).sum())
    assert definite.sum() > 1000 and (~definite).sum() > 100, (definite.sum(), (~definite).sum())
    assert mixed >= 1, "no tile holds both classes"
    needle = (gid >= N) & (gid < N + NEEDLES)
    # the needles are what the classifier rejects (but for those seen end on)
    assert needle.sum() > 1000 and definite[needle].mean() < 0.5 < definite[~needle].mean(), definite[needle].mean()
    # batches of both kinds: 64-instance batches (forward order) that are all definite, and ones that are not
    kinds = {True: 0, False: 0}
    for t in range(gx * gx):
        d = definite[tile_of == t]
        for b in range(0, len(d), 64):
            kinds[bool(d[b: b + 64].all())] += 1
    assert kinds[True] >= 10 and kinds[False] >= 10, kinds
    # the on-centre Gaussian: loaded, definite, exactly on its pixel, which composites it (power2 = 0 is taken)
    assert (hs["xy"][centre] == pixel).all() and definite[gid == centre].all() and (gid == centre).any()
    assert hs["n_contrib"][int(pixel[1]), int(pixel[0])] > 0
    # opacities on both sides of the clamp are among the loaded instances, and just above 1/255 (alpha passes within a
    # pixel or two of the centre only); those below 1/255 are in the scene, where the preprocess gives them no tile
    o = co[:, 3]
    assert (o > 0.99).any() and (o == 1.0).any() and (o < 2.0 / 255.0).any()
    assert (inp["opacities"][LOW] < 1.0 / 255.0).sum() > 30 and not (o < 1.0 / 255.0).any()


@pytest.mark.parametrize("ext", [False, True], ids=["plain", "ext"])
@pytest.mark.parametrize("knobs", [dict(), dict(fwd_parts=1, bwd_parts=1, bwd_seg=0), dict(fwd_parts=2, bwd_seg=0),
                                   dict(bwd_seg=0, bwd_parts=1, bwd_union=1)],
                         ids=["default", "whole", "parts", "union"])
def test_definite_fast_is_bitwise_the_generic_body(gpu_device, knobs, ext):
    from gaussian_splatting_lightning_amd import _native
    whole = knobs.get("fwd_parts") == 1
    with _native.tuned(definite_fast=0, **knobs):
        want, _ = _render(gpu_device, ext, whole)
    with _native.tuned(definite_fast=1, **knobs):
        got, _ = _render(gpu_device, ext, whole)
    assert set(got) == set(want) and {"color", "invdepth", "radii", "final_T", "n_contrib", "grad_means3D",
                                      "grad_means2D", "grad_opacities", "grad_scales", "grad_rotations",
                                      "grad_shs"} <= set(got), sorted(got)
    assert ("strip_mask" in got) == whole and ("alpha" in got) == ext
    for k in want:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    # the comparison is of real work: gradients that are not all zero, pixels that composited something
    assert np.count_nonzero(want["grad_means2D"]) > 1000 and np.count_nonzero(want["n_contrib"]) > W * H // 2
