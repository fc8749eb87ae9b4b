"""The edge scenes of tests/edge_cases.py on the CPU: a census that each scene reaches the branch it is for, the oracle
against the reference's fixture (tests/golden/edges.npz, tests/golden/make_golden_edges.py) and the antialiasing
floor's equivalence on the oracle.  tests/test_edge_parity.py runs the same scenes through the HIP path.

The census counts are conditions on the inputs, met by tuning the builders against the oracle alone: they say that
the scene takes the branch, not how well anything computes it.  Bars of the comparisons: the project's existing ones
(tests/helpers.py compare_to_reference, test_golden_unsaturated_direct's 1e-5 / 1e-4; COLOR_TOL and GRAD_CLEAN_TOL of
tests/test_gpu_parity.py for the floor equivalence, whose two sides are one rasterizer on equivalent inputs)."""
import functools

import numpy as np
import pytest

from tests import edge_cases as E
from tests.helpers import FLIP_EXCLUDE, rel_l2, run_oracle
from tests.test_gpu_parity import COLOR_TOL, GRAD_CLEAN_TOL

GRADS = E.GRAD_KEYS


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """(inputs, extras, oracle outputs) of one case before any mask, computed once."""
    full, dc, di = E.build(name)
    inp = E.rasterizer_inputs(full)
    return inp, full, dc, di, run_oracle(inp, antialiasing=E.antialiased(name))


@functools.lru_cache(maxsize=None)
def _census(name):
    inp, _, _, _, out = _oracle(name)
    return E.pair_census(out[3], inp)


# ---- census ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", E.CASES)
def test_census_every_case(name):
    """At most 600 Gaussians; threshold-flip candidate pixels are at most 2 % of the image; the Gaussians no candidate
    pixel's walk reaches are at least half of the rendered ones (so the clean-gradient bar speaks for the scene)."""
    inp, _, _, _, (_, radii, _, run) = _oracle(name)
    assert len(radii) <= 600
    assert (inp["image_width"], inp["image_height"]) == ((E.NEAR_W, E.NEAR_H) if name == "near_plane" else (E.W, E.H))
    assert inp["sh_degree"] == (3 if name == "rotations" else 1) and inp["shs"].shape[1] == (inp["sh_degree"] + 1) ** 2
    cand = run.threshold_margin() < FLIP_EXCLUDE
    rendered = run.geom()["tiles_touched"] > 0
    touched = E.flip_touched(run, inp)
    print(name, "candidates", int(cand.sum()), "of", cand.size, "touched", int(touched.sum()), "rendered",
          int(rendered.sum()))
    assert cand.sum() <= 0.02 * cand.size
    assert rendered.sum() >= 100
    assert (rendered & ~touched).sum() >= 0.5 * rendered.sum()


def test_census_alpha_clamp():
    """At least 200 (Gaussian, pixel) pairs with o G > 0.99 on kept pixels, from at least 20 Gaussians; o spans
    [0.99, 1.0] with exactly 1.0f; no kept pixel is stopped by either termination rule -- from the oracle's state: its
    final transmittance is the product over ALL of the tile's instances and its contributor count reaches the last
    instance with alpha >= 1/255 (a stopped walk would leave both short)."""
    inp, full, _, _, (_, _, _, run) = _oracle("alpha_clamp")
    c = _census("alpha_clamp")
    kept = E.kept_mask("alpha_clamp", run, inp, c)
    pairs = c["clamped_pixels"]
    on_kept = kept[pairs[:, 1], pairs[:, 2]]
    gaussians = np.unique(pairs[on_kept, 0])
    print("clamped pairs", len(pairs), "on kept pixels", int(on_kept.sum()), "from", len(gaussians), "Gaussians; kept",
          int(kept.sum()), "of", kept.size)
    assert on_kept.sum() >= 200 and len(gaussians) >= 20
    assert set(gaussians) <= set(full["opaque_idx"])
    o = inp["opacities"][full["opaque_idx"], 0]
    assert o.min() == np.float32(0.99) and o.max() == np.float32(1.0) and len(o) == E.ALPHA_CLAMP_OPAQUE
    ft, nc = run.image_state()
    assert ft[kept].min() >= E.T_KEEP_EDGE * (1 - 1e-4)
    assert np.abs(ft / c["T_all"] - 1.0)[kept].max() <= 1e-4
    assert np.array_equal(nc[kept], c["last"][kept])
    assert kept.mean() >= 0.95
    # every clamped kept pixel lies below tests/helpers.py T_KEEP: that mask would have dropped them all
    assert c["T_all"][kept & (c["clamped"] > 0)].max() <= 0.01


@pytest.mark.parametrize("name", ["aa_floor_all", "aa_floor_mixed"])
def test_census_aa_floor(name):
    inp, full, _, _, (_, _, _, run) = _oracle(name)
    p = E.project64(inp)
    rendered = run.geom()["tiles_touched"] > 0
    on_floor = p["ratio"] <= E.AA_FLOOR
    print(name, "rendered on the floor", int((rendered & on_floor).sum()), "above", int((rendered & ~on_floor).sum()))
    assert (rendered & on_floor).sum() >= 100
    assert np.array_equal(np.nonzero(on_floor)[0], full["floor_idx"])
    assert p["ratio"][on_floor].max() <= 0.1 * E.AA_FLOOR  # not near the floor's edge in fp32
    if name == "aa_floor_all":
        assert on_floor.all()
    else:
        assert (rendered & ~on_floor).sum() >= 100 and p["ratio"][~on_floor].min() >= 10 * E.AA_FLOOR
    o = inp["opacities"]
    assert o.min() >= 0.8 and o.max() <= 0.999 and o.min() * float(E.AA_FLOOR_H) >= 1.0 / 255.0


def test_census_near_plane():
    inp, _, _, _, (_, radii, _, run) = _oracle("near_plane")
    z = E.project64(inp)["z"]
    tiles = run.geom()["tiles_touched"]
    print("behind", int((z <= E.NEAR).sum()), "in front", int((z > E.NEAR).sum()), "z", z.min(), z.max(),
          "kept above 64 tiles", int((tiles > E.BIG_GAUSSIAN_TILES).sum()))
    assert 0.12 <= z.min() < z.max() <= 0.35
    assert (z <= E.NEAR).sum() >= 20 and (z > E.NEAR).sum() >= 20
    assert np.abs(z - E.NEAR).min() >= 1e-4
    assert (tiles > E.BIG_GAUSSIAN_TILES).sum() >= 5
    assert not radii[z <= E.NEAR].any() and (radii[z > E.NEAR] > 0).mean() > 0.8


def test_census_cameras():
    """The five cameras differ from the generator's family in the way their names say."""
    cam = {name: _oracle(name)[0] for name in E.CAMERAS}
    assert cam["cam_wide"]["tanfovx"] == 1.5 and cam["cam_narrow"]["tanfovx"] == 0.08
    a = cam["cam_anamorphic"]
    assert np.isclose(a["tanfovy"], 1.4 * a["tanfovx"] * E.H / E.W)
    for name, inp in cam.items():  # the projection matches the field of view
        P = np.linalg.inv(inp["viewmatrix"].astype(np.float64)) @ inp["projmatrix"].astype(np.float64)
        assert np.isclose(P[0, 0], 1.0 / inp["tanfovx"], rtol=1e-5)
        assert np.isclose(P[1, 1], 1.0 / inp["tanfovy"], rtol=1e-5)
        off = (0.4, -0.3) if name == "cam_offcentre" else (0.0, 0.0)  # (0.2 W, -0.15 H) pixels in NDC units
        assert np.allclose(P[2, :2], off, atol=1e-5), name
    from gaussian_splatting_lightning_amd.synthetic import TREEHILL_V0
    R = cam["cam_rolled"]["viewmatrix"][:3, :3].astype(np.float64).T @ np.asarray(TREEHILL_V0)[:3, :3]
    assert np.degrees(np.arccos((np.trace(R) - 1) / 2)) > 37.0  # the roll and the pitch compose


def test_census_rotations():
    inp, full, _, _, (_, _, _, run) = _oracle("rotations")
    rendered = run.geom()["tiles_touched"] > 0
    kind, q, s = full["kind"], inp["rotations"], inp["scales"]
    counts = [int((rendered & (kind == k)).sum()) for k in range(3)]
    print("rendered per third", counts)
    assert min(counts) >= 50
    assert np.all(q[kind == 0] == np.array([1, 0, 0, 0], np.float32)) and np.all(s[kind == 0] == s[kind == 0][:, :1])
    n1 = np.linalg.norm(q[kind == 1].astype(np.float64), axis=1)
    assert n1.min() >= 0.499 and n1.max() <= 2.001 and (np.abs(n1 - 1) > 0.05).mean() > 0.8
    assert np.allclose(np.linalg.norm(q[kind == 2].astype(np.float64), axis=1), 1.0, atol=1e-6)


def test_census_extremes():
    inp, full, _, _, (_, _, _, run) = _oracle("extremes")
    o, cls = inp["opacities"][:, 0], full["class"]
    third = np.float32(1.0) / np.float32(255.0)
    rendered = run.geom()["tiles_touched"] > 0
    assert (o == 0).sum() >= 10 and (o == np.float32(1.0)).sum() >= 3
    below, above = (o < third) & (o > 0.999 * float(third) - 1e-6), (o > third) & (o < 1.0011 * float(third))
    assert below.sum() >= 10 and above.sum() >= 10
    assert np.allclose(o[below], float(third) * (1 - 1e-3), rtol=1e-6)
    assert np.allclose(o[above], float(third) * (1 + 1e-3), rtol=1e-6)
    assert not rendered[(o == 0) | below].any()      # alpha < 1/255 everywhere: exact culling keeps no tile
    assert rendered[o == np.float32(1.0)].all() and rendered[above].any()
    p = E.project64(inp)
    gx, gy = p["grid"]
    whole = (p["rect"] == np.array([0, 0, gx, gy])).all(1)
    print("rectangles equal to the grid", int(whole.sum()), "of them class 4:", int((whole & (cls == 4)).sum()))
    assert whole.sum() >= 3
    # clamped on all four sides: the unclamped rectangle sticks out everywhere
    big = np.nonzero(whole)[0]
    assert np.all(p["pix"][big, 0] - p["radius"][big] < 0) and np.all(p["pix"][big, 0] + p["radius"][big] > E.W)
    assert np.all(p["pix"][big, 1] - p["radius"][big] < 0) and np.all(p["pix"][big, 1] + p["radius"][big] > E.H)


# ---- the oracle against the reference's fixture ------------------------------------------------------------------------
@pytest.mark.parametrize("name", E.REF_CASES + E.REF_FORWARD_ONLY)
def test_oracle_against_reference(name):
    """The oracle against the reference Python rasterizer's outputs and autograd gradients on the edge scenes
    (alpha_clamp: against the reference with the pass-through clamp gradient of upstream CUDA, and farther than 1e-3
    from the unmodified reference's dL/dopacities -- Appendix A15).  Achieved (relative L2 of the six gradients):
    <= 3.5e-6 on every case."""
    z = E.load_case(name)
    aa = E.antialiased(name)
    color, radii, invd, run = run_oracle(z["inp"], antialiasing=aa)
    ft, _ = run.image_state()
    mask = E.kept_mask(name, run, z["inp"])
    assert np.array_equal(mask, z["mask"]), "the fixture's mask is the oracle's"
    rgb_max = float(np.abs(run.geom()["rgb"][radii > 0]).max())
    g = run.backward(z["dL_dcolor"], z["dL_dinvdepth"]) if name in E.REF_CASES else None
    rec = E.compare_with_fixture(z, color, invd, radii, ft, rgb_max, run.threshold_margin(), g)
    print(name, {k: v for k, v in rec.items() if k.startswith(("grad_", "color_", "invdepth_"))})
    if name == "alpha_clamp":
        away = rel_l2(g["opacities"], z["plain_grad_opacities"])
        print("dL/dopacities against the unmodified reference:", away, "dL/dmeans3D:",
              rel_l2(g["means3D"], z["plain_grad_means3D"]))
        assert away > 1e-3


# ---- the antialiasing floor's equivalence on the oracle ---------------------------------------------------------------
def floor_equivalence(aa: dict, plain: dict, record=None) -> dict:
    """aa_floor_all rendered with antialiasing (every Gaussian's opacity factor is sqrtf(2.5e-5f), a constant: the
    floor branch, d_inside_root = 0) against the same scene without antialiasing and opacities o sqrtf(2.5e-5f).  The
    non-antialiased path is the one pinned to the reference, so this pins the floor branch without a reference
    backward.  aa / plain: dicts with color, invdepth, radii, grads."""
    h = float(E.AA_FLOOR_H)
    rec = dict(color_maxabs=float(np.abs(aa["color"] - plain["color"]).max()),
               invdepth_maxrel=float((np.abs(aa["invdepth"] - plain["invdepth"]) /
                                      np.maximum(np.abs(plain["invdepth"]), 1.0)).max()),
               radii_equal=bool(np.array_equal(aa["radii"], plain["radii"])))
    for k in GRADS:
        rec["grad_" + k] = rel_l2(aa["grads"][k], plain["grads"][k] * (h if k == "opacities" else 1.0))
    if record is not None:
        record(rec)
    assert rec["radii_equal"], rec
    assert rec["color_maxabs"] <= COLOR_TOL and rec["invdepth_maxrel"] <= COLOR_TOL, rec
    for k in GRADS:
        assert rec["grad_" + k] <= GRAD_CLEAN_TOL, (k, rec)
    assert np.linalg.norm(plain["grads"]["opacities"]) > 0 and np.linalg.norm(plain["grads"]["scales"]) > 0
    return rec


def test_oracle_floor_equivalence():
    inp, _, dc, di, (color, radii, invd, run) = _oracle("aa_floor_all")
    pc, pr, pi, prun = run_oracle(E.floor_equivalent(inp), antialiasing=False)
    rec = floor_equivalence(dict(color=color, invdepth=invd, radii=radii, grads=run.backward(dc, di)),
                            dict(color=pc, invdepth=pi, radii=pr, grads=prun.backward(dc, di)))
    print(rec)


def test_oracle_near_plane_culled_are_zero():
    inp, _, dc, di, (_, radii, _, run) = _oracle("near_plane")
    culled = E.project64(inp)["z"] <= E.NEAR
    g = run.backward(dc, di)
    assert not radii[culled].any()
    for k in GRADS:
        assert not g[k][culled].any(), k
        assert g[k][~culled].any(), k
