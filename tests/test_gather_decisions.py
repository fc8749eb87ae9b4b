"""The backward's per-Gaussian gathers -- the 40-B rows (preprocess_bwd_kernel, both its per-lane and its wave-joint
form), the 8-B abs rows (abs_gather_kernel) and the feature rows (feat_gather_kernel) -- decide which rows to add from
the same four facts (GatherSrc, gsr_gather.h): a positive radius, the live flag when the validity word says the last
composite set it, more than 64 kept tiles (the block-reduced sum), and the inv word of each instance.  One scene at the
smallest shape where every branch occurs, 144x144 (81 tiles) and 187 Gaussians; gather_scene() builds it and its census
is asserted from the device's own state, so a change of the scene helpers that loses a branch fails here."""
import numpy as np
import pytest
import torch

from gaussian_splatting_lightning_amd.synthetic import make_camera, make_scene
from tests.helpers import hip_state_arrays, settings_for, upstream

W = H = 144
N_RANDOM, N_STACK = 64, 120
SPECIAL = dict(culled=0, big=1, occluded=2)  # indices of the hand-placed Gaussians, in front of the stack and the rest
INV_NONE = 0xFFFFFFFF
GRADS = ("means3D", "means2D", "opacities", "scales", "rotations", "shs")
pytestmark = pytest.mark.gpu


def gather_scene(sh_degree):
    """Scene inputs (tests.helpers.scene_inputs' dict).  Hand-placed, isotropic, by pixel position, pixel sigma and view
    depth: [0] behind the camera (radius 0); [1] sigma 40 px over the image centre, in front of everything, faint
    (all 81 tiles: the big-Gaussian path); [2] a 1-px dot behind the stack (visible, but no pixel takes it);
    [3 : 3 + N_STACK] a stack of nearly opaque sigma-12 Gaussians over the centre of tile (4, 4), which saturates that
    tile after a few of them, so the rest of the tile's instances are never loaded (inv stays INV_NONE).  Then N_RANDOM
    Gaussians of make_scene, whose kept-tile counts include 1, 2, 3 and 5."""
    cam = make_camera(W, H)
    inv_view = torch.linalg.inv(cam.viewmatrix)
    focal = W / (2.0 * cam.tanfovx)

    def place(px, py, z, sigma_px, opacity):
        xn, yn = (2 * px + 1) / W - 1, (2 * py + 1) / H - 1
        pv = torch.tensor([xn * z * cam.tanfovx, yn * z * cam.tanfovy, z, 1.0])
        return (pv @ inv_view)[:3], sigma_px * abs(z) / focal, opacity

    hand = [place(72, 72, -1.0, 2.0, 0.5), place(72, 72, 2.0, 40.0, 0.05), place(72, 72, 5.0, 1.0, 0.9)]
    hand += [place(72, 72, 3.0 + 0.001 * k, 12.0, 0.99) for k in range(N_STACK)]
    sc = make_scene(N_RANDOM, sh_degree=sh_degree, seed=5)
    n = len(hand) + N_RANDOM
    g = torch.Generator().manual_seed(6)
    means = torch.cat([torch.stack([h[0] for h in hand]), sc.means3D])
    scales = torch.cat([torch.tensor([[h[1]] * 3 for h in hand]), sc.scales])
    rots = torch.cat([torch.tensor([[1.0, 0.0, 0.0, 0.0]] * len(hand)), sc.rotations])
    opac = torch.cat([torch.tensor([[h[2]] for h in hand]), sc.opacities])
    shs = torch.cat([torch.randn(len(hand), (sh_degree + 1) ** 2, 3, generator=g) * 0.3, sc.shs])
    f32 = lambda t: np.ascontiguousarray(t.numpy(), np.float32)  # noqa: E731
    assert means.shape[0] == n
    return dict(means3D=f32(means), opacities=f32(opac), scales=f32(scales), rotations=f32(rots), shs=f32(shs),
                viewmatrix=f32(cam.viewmatrix), projmatrix=f32(cam.projmatrix), campos=f32(cam.campos),
                bg=np.zeros(3, np.float32), tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, image_height=H, image_width=W,
                sh_degree=sh_degree, scale_modifier=1.0)


def census(radii, tiles, inst_start, inv, tile_loaded, ranges):
    """What the scene must contain, from a forward's state (the device's, or the oracle's restated): asserts it."""
    assert radii[SPECIAL["culled"]] == 0
    assert tiles[SPECIAL["big"]] > 64, tiles[SPECIAL["big"]]
    occ = SPECIAL["occluded"]
    assert radii[occ] > 0 and tiles[occ] >= 1
    assert np.all(inv[inst_start[occ]: inst_start[occ] + tiles[occ]] == INV_NONE)  # never loaded: no pixel took it
    kept = set(int(t) for t, r in zip(tiles, radii) if r > 0)
    assert {1, 2, 3, 5} <= kept, sorted(kept)
    lens = ranges[:, 1].astype(np.int64) - ranges[:, 0]
    assert np.any((tile_loaded > 0) & (tile_loaded < lens)), "no tile saturates before its list ends"
    assert np.any(inv == INV_NONE) and np.any(inv != INV_NONE)


@pytest.fixture(scope="module", params=[3, 1], ids=["sh3_joint_gather", "sh1_per_lane_gather"])
def scene(request, gpu_device):
    """The scene on the device, its upstream gradients, and the plain forward + backward every test compares with.
    SH degree 3 (16 coefficients) takes preprocess_bwd_kernel's wave-joint gather, degree 1 its per-lane loop."""
    from gaussian_splatting_lightning_amd.rasterizer import backward_raw, forward_raw
    inp = gather_scene(request.param)
    rs = settings_for(inp, gpu_device)
    t = {k: torch.as_tensor(inp[k], device=gpu_device) for k in ("means3D", "opacities", "scales", "rotations", "shs")}
    args = (t["means3D"], t["shs"], None, t["opacities"], t["scales"], t["rotations"], None, rs)
    dc, di = (torch.as_tensor(a, device=gpu_device) for a in upstream(W, H, 41))
    color, radii, invd, st = forward_raw(*args)
    plain = backward_raw(st, rs, dc, di)
    torch.cuda.synchronize()
    return dict(inp=inp, rs=rs, args=args, dc=dc, di=di, st=st, plain=plain, n=inp["means3D"].shape[0],
                out=dict(color=color.cpu().numpy(), radii=radii.cpu().numpy(), invdepth=invd.cpu().numpy(), state=st))


def _same(got, want, keys=GRADS):
    for k in keys:
        assert torch.equal(got[k], want[k]), k


def test_scene_has_every_branch(scene):
    from gaussian_splatting_lightning_amd import _native
    s = hip_state_arrays(scene["out"])
    st = scene["st"]
    lay = _native.state_layout(scene["n"], st.num_rendered, W, H)
    off = lay["geom_inst_start"]
    inst_start = st.geom_buffer[off: off + 4 * (scene["n"] + 1)].view(torch.int32).cpu().numpy().astype(np.int64)
    census(scene["out"]["radii"], s["tiles"].astype(np.int64), inst_start, s["inv"], s["tile_loaded"].astype(np.int64),
           s["ranges"])
    assert st.num_big >= 1
    g = scene["plain"]
    for k in GRADS:  # the occluded Gaussian and the culled one: exact zeros
        for i in (SPECIAL["occluded"], SPECIAL["culled"]):
            assert not torch.any(g[k][i]), (k, i)
    assert torch.any(g["means2D"][SPECIAL["big"]])


def test_plain_absgrad_and_features_agree(scene):
    """dL/d* keep their bits with the abs gather beside them, with a state that carries features and no feature
    gradient, and with an all-zero feature gradient, which runs the feature walk and gather of every channel block
    (C = 3: one block of 8; C = 9: a block of 16) and adds exact zeros to the rows."""
    from gaussian_splatting_lightning_amd.rasterizer import backward_raw, forward_raw
    rs, dc, di, plain, n = (scene[k] for k in ("rs", "dc", "di", "plain", "n"))
    _same(backward_raw(scene["st"], rs, dc, di, absgrad=True), plain)
    for C in (3, 9):
        f = torch.randn(n, C, generator=torch.Generator().manual_seed(C)).to(dc.device)
        stf = forward_raw(*scene["args"], features=f)[-1]
        _same(backward_raw(stf, rs, dc, di), plain)
        g = backward_raw(stf, rs, dc, di, grad_out_features=torch.zeros(C, H, W, device=dc.device))
        _same(g, plain)
        assert not torch.any(g["features"])


def test_abs_and_feature_gathers_do_not_depend_on_the_live_flags(scene):
    """means2D_abs and dL/dfeatures (C = 3 and 9, under a real feature gradient), and every other gradient of those
    calls, are the same with the live flags ("bwd_live" 1) and with every Gaussian gathered (0)."""
    from gaussian_splatting_lightning_amd import _native
    from gaussian_splatting_lightning_amd.rasterizer import backward_raw, forward_raw
    rs, dc, di, n = (scene[k] for k in ("rs", "dc", "di", "n"))
    calls = [(scene["st"], dict(absgrad=True), "means2D_abs")]
    for C in (3, 9):
        gen = torch.Generator().manual_seed(10 + C)
        f = torch.randn(n, C, generator=gen).to(dc.device)
        dF = torch.randn(C, H, W, generator=gen).to(dc.device)
        calls.append((forward_raw(*scene["args"], features=f)[-1], dict(grad_out_features=dF), "features"))
    for st, kw, name in calls:
        res = {}
        for knob in (1, 0):
            with _native.tuned(bwd_live=knob):
                res[knob] = backward_raw(st, rs, dc, di, **kw)
        _same(res[1], res[0], GRADS + (name,))
        assert torch.any(res[1][name])
        for i in (SPECIAL["occluded"], SPECIAL["culled"]):
            assert not torch.any(res[1][name][i]), (name, i)


def test_split_stages_with_unmarked_composite(scene):
    """After a marked backward on the same forward (its upstream gradient zero on half the image), GSR_BWD_COMPOSITE
    under "bwd_live" 0 marks nothing and clears the validity word, and GSR_BWD_GAUSSIANS under "bwd_live" 1 reads the
    flags' pointer: the per-Gaussian gathers (the abs gather with them) must not trust the stale flags.  Bitwise a
    fresh forward + backward."""
    from gaussian_splatting_lightning_amd import _native
    from gaussian_splatting_lightning_amd.rasterizer import backward_chunked, backward_raw, forward_raw
    rs, dc, di, n = (scene[k] for k in ("rs", "dc", "di", "n"))
    d1, i1 = dc.clone(), di.clone()
    d1[:, :, W // 2:] = 0.0
    i1[:, :, W // 2:] = 0.0
    M = scene["inp"]["shs"].shape[1]
    widths = dict(means3D=3, means2D=3, opacities=1, scales=3, rotations=4, shs=3 * M, means2D_abs=2)
    st = forward_raw(*scene["args"])[-1]
    backward_raw(st, rs, d1, i1)  # marks the left half's Gaussians
    out = {k: torch.full((n, w), float("nan"), device=dc.device) for k, w in widths.items()}
    with _native.tuned(bwd_live=0):
        backward_chunked(st, rs, dc, di, [(0, n, out)], after_composite=lambda: _native.set_tuning("bwd_live", 1))
    fresh = backward_raw(forward_raw(*scene["args"])[-1], rs, dc, di, absgrad=True)
    torch.cuda.synchronize()
    for k in widths:
        assert torch.equal(out[k].reshape(fresh[k].shape), fresh[k]), k
    _same(fresh, scene["plain"])
