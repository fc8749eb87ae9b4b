"""The edge scenes of tests/edge_cases.py through the HIP path: the clamp and cut-off branches no other fixture reaches
(alpha = min(0.99, o G), the antialiasing floor, the near-plane cull, cameras outside the generator's family, identity
and non-unit quaternions, opacities at 0, 1/255 and 1, tile rectangles clamped to the whole grid).

  * HIP against the oracle on every case, through tests/test_gpu_parity.py's compare_forward / compare_backward
    unchanged (bit-exact integer state and render records, COLOR_TOL, GRAD_CLEAN_TOL, the derived all-Gaussian bar,
    and GRAD_CLEAN_TOL over all Gaussians with the flip candidates' upstream gradients masked where a case has any),
    under four selections so that every composite kernel sees the edges: the default (segmented walk at these image
    sizes), the threshold guard, the whole-tile walk and the part-wave walk;
  * HIP against the reference's fixture tests/golden/edges.npz with the reference bars of the CPU leg
    (tests/edge_cases.py compare_with_fixture); alpha_clamp also stays farther than 1e-3 from the UNMODIFIED
    reference's dL/dopacities, so a silent change of the clamp-gradient convention fails;
  * the antialiasing floor's equivalence (tests/test_edge_cases.py floor_equivalence);
  * near_plane: culled Gaussians have radius 0 and exactly zero gradients in every output.
No bar here is fitted to HIP or oracle output.  Achieved figures: profiles/parity_edges.json."""
import functools

import numpy as np
import pytest

from tests import edge_cases as E
from tests import parity
from tests.helpers import hip_state_arrays, rel_l2, run_hip, run_oracle
from tests.test_edge_cases import floor_equivalence
from tests.test_gpu_parity import GRADS, _case, compare_backward, compare_forward, flip_candidates

pytestmark = pytest.mark.gpu

SELECTIONS = {"default": {}, "guard": dict(guard=1), "whole_tile": dict(bwd_seg=0, bwd_parts=1),
              "part_waves": dict(bwd_seg=0, bwd_parts=4)}
GUARD_GRAD_TOL = 1e-5  # all-Gaussian gradient bar under the guard (test_threshold_guard_band)


@functools.lru_cache(maxsize=None)
def _scene(name):
    """(inputs, dL_dcolor, dL_dinvdepth, the oracle's forward) of one case, computed once for the four selections."""
    full, dc, di = E.build(name)
    inp = E.rasterizer_inputs(full)
    return inp, dc, di, run_oracle(inp, antialiasing=E.antialiased(name))


@pytest.mark.parametrize("selection", list(SELECTIONS))
@pytest.mark.parametrize("name", E.CASES)
def test_edge_case_vs_oracle(gpu_device, name, selection):
    from gaussian_splatting_lightning_amd import _native
    inp, dc, di, oracle_out = _scene(name)
    with _native.tuned(**SELECTIONS[selection]):
        hip = run_hip(inp, gpu_device, dc, di, antialiasing=E.antialiased(name),
                      flip_mask=flip_candidates(oracle_out[3]))  # the masked backward under this selection too
    run = compare_forward(inp, hip, oracle_out)
    g = compare_backward(hip, run, dc, di)
    if selection == "guard":
        err = {k: rel_l2(hip["grads"][k], g[k]) for k in GRADS}
        parity.record(_case(), "guard_all_gaussians", err)
        for k, e in err.items():
            assert e <= GUARD_GRAD_TOL, (k, e)


@pytest.mark.parametrize("name", E.REF_CASES + E.REF_FORWARD_ONLY)
def test_edge_case_vs_reference(gpu_device, name):
    z = E.load_case(name)
    backward = name in E.REF_CASES
    hip = run_hip(z["inp"], gpu_device, z["dL_dcolor"] if backward else None, z["dL_dinvdepth"] if backward else None,
                  antialiasing=E.antialiased(name))
    hs = hip_state_arrays(hip)
    rgb_max = float(np.abs(hs["rec"].view(np.float32)[:, 6:9]).max())
    margin = run_oracle(z["inp"], antialiasing=E.antialiased(name))[3].threshold_margin()  # names the flip candidates
    E.compare_with_fixture(z, hip["color"], hip["invdepth"], hip["radii"], hs["final_T"], rgb_max, margin,
                           hip["grads"] if backward else None,
                           record=lambda r: parity.record(_case(), "reference", r))
    if name == "alpha_clamp":
        away = {k: rel_l2(hip["grads"][k], z["plain_grad_" + k]) for k in GRADS}
        parity.record(_case(), "unmodified_reference", away)
        assert away["opacities"] > 1e-3, away


def test_aa_floor_equivalence(gpu_device):
    inp, dc, di, _ = _scene("aa_floor_all")
    aa = run_hip(inp, gpu_device, dc, di, antialiasing=True)
    plain = run_hip(E.floor_equivalent(inp), gpu_device, dc, di, antialiasing=False)
    floor_equivalence(aa, plain, record=lambda r: parity.record(_case(), "floor_equivalence", r))


def test_near_plane_culled_are_zero(gpu_device):
    inp, dc, di, _ = _scene("near_plane")
    hip = run_hip(inp, gpu_device, dc, di)
    culled = E.project64(inp)["z"] <= E.NEAR
    assert culled.sum() >= 20 and not hip["radii"][culled].any()
    for k in GRADS:
        assert not hip["grads"][k][culled].any(), k
        assert hip["grads"][k][~culled].any(), k
