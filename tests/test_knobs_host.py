"""The knob table (csrc/gsr_knobs.def) through the C boundary and _native, the parts that need no GPU: the list of
names, set / get / unset of every knob, the refusal of unknown, read-only and retired names (by the library, by
tuned() before it changes anything, and by GSR_TUNE at load), the three list functions in the header and the exports,
and that every knob a variant test selects is one the library has."""
import importlib
import inspect
import os
import re
import subprocess
import sys

import pytest

from gaussian_splatting_lightning_amd import _native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "gsrast.h")
# retired with their code paths (DESIGN.md §4 "Knobs."): none may come back under its old name
RETIRED = ("seg32", "seg_minw", "seg_grid", "bk_colw", "bk_colt", "bk_blocks", "lbw", "tile_lo_short", "rs_items",
           "lpt_multi_tiles", "lpt_shift", "lpt_append", "fwd_part_slots", "bwd_part_slots", "bin_prealloc", "rb_spin",
           "lb_patience",
           "bwd_lastc", "bwd_order", "exp_owner", "pre_late", "pre_late_minw", "pre_shd", "pre_split", "rs_cs64",
           "scan_lookback", "sh_vec16", "sort_gather", "views_staged", "zero_kernel")
UNSET = _native.TUNING_UNSET


def _names():
    lib = _native.load()
    return [lib.gsr_tuning_name(i).decode() for i in range(lib.gsr_num_tunings())]


def _is_unset(name):
    return _native.get_tuning(name, 17) == 17 and _native.get_tuning(name, -23) == -23


def test_names_are_unique_and_no_statistic_is_a_knob():
    lib, names = _native.load(), _names()
    assert len(names) == lib.gsr_num_tunings() > 0 and len(set(names)) == len(names)
    for n in names:
        assert n and re.fullmatch(r"[a-z][a-z0-9_]*", n) and not n.startswith("stat_"), n
    assert _native.tunings() == {n: lib.gsr_tuning_default(i) for i, n in enumerate(names)}
    assert _native.tunings()["onesweep_max_n"] == 3 << 20 and _native.tunings()["bwd_union"] == -1
    for i in (-1, len(names)):
        assert lib.gsr_tuning_name(i) == b"" and lib.gsr_tuning_default(i) == 0


def test_every_knob_round_trips():
    for name in _names():
        assert _is_unset(name), name
        for v in (5, 0, -1):  # 0 and -1 are values like any other, not "unset"
            _native.set_tuning(name, v)
            assert _native.get_tuning(name, 17) == v and _native.get_tuning(name, -23) == v, (name, v)
        _native.unset_tuning(name)
        assert _is_unset(name), name
        with _native.tuned(**{name: 9}):
            assert _native.get_tuning(name, 17) == 9
            with _native.tuned(**{name: 4}):
                assert _native.get_tuning(name, 17) == 4
            assert _native.get_tuning(name, 17) == 9  # the earlier value, not the default
        assert _is_unset(name), name


@pytest.mark.parametrize("name", ["no_such_knob", "stat_depth_passes", "Bucket", "bucket ", ""])
def test_unknown_and_read_only_names_are_refused(name):
    lib = _native.load()
    before = _native.get_tuning(name, 17), _native.get_tuning(name, -23)  # (a statistic has a value after a forward)
    for call in (lambda: _native.set_tuning(name, 1), lambda: _native.unset_tuning(name)):
        with pytest.raises(KeyError) as e:
            call()
        assert f'"{name}"' in str(e.value)
    assert lib.gsr_set_tuning(name.encode(), 1) == 1  # GSR_ERR_ARG
    assert f'"{name}"' in lib.gsr_last_error().decode()
    assert lib.gsr_set_tuning(None, 1) == 1
    assert (_native.get_tuning(name, 17), _native.get_tuning(name, -23)) == before  # nothing left behind
    assert before == (17, -23) or name.startswith("stat_")
    assert lib.gsr_set_tuning(b"bucket", UNSET) == 0


def test_tuned_refuses_before_it_changes_anything():
    for knobs in (dict(bucket=2, no_such_knob=1), dict(no_such_knob=1, bucket=2), dict(bucket=2, stat_depth_passes=1)):
        with pytest.raises(KeyError) as e:
            with _native.tuned(**knobs):
                raise AssertionError("the body must not run")
        assert next(k for k in knobs if k != "bucket") in str(e.value)
        assert _is_unset("bucket")


@pytest.mark.parametrize("name", RETIRED)
def test_retired_names_are_refused(name):
    assert name not in _names()
    with pytest.raises(KeyError):
        _native.set_tuning(name, 1)
    assert _is_unset(name)


def _child(tune, code):
    env = dict(os.environ, GSR_TUNE=tune, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-c", "from gaussian_splatting_lightning_amd import _native\n" + code],
                          env=env, cwd=REPO, capture_output=True, text=True, timeout=120)


def test_gsr_tune_is_checked_at_load():
    r = _child("guard=1,seg_k=32", "_native.load()\nprint(_native.get_tuning('guard', 0), _native.get_tuning('seg_k', 0), "
               "_native.get_tuning('bucket', 7))")
    assert r.returncode == 0 and r.stdout.split() == ["1", "32", "7"], r.stderr
    r = _child("guard=1,no_such_knob=1", "_native.load()")
    assert r.returncode != 0 and "KeyError" in r.stderr and "no_such_knob" in r.stderr, r.stderr


def test_header_and_exports():
    lib = _native.load()
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for decl in (r"int gsr_set_tuning\(const char \*name, int value\);", r"int gsr_get_tuning\(const char \*name, int default_value\);",
                 r"int gsr_num_tunings\(void\);", r"const char \*gsr_tuning_name\(int i\);", r"int gsr_tuning_default\(int i\);"):
        assert re.search(decl, header), decl
    for name in ("gsr_num_tunings", "gsr_tuning_name", "gsr_tuning_default", "gsr_set_tuning", "gsr_get_tuning"):
        assert name in _native.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert "#define GSR_TUNING_UNSET (-2147483647 - 1)" in header and UNSET == -2 ** 31
    assert lib.gsr_abi_version() == _native.ABI_VERSION == 3  # new entry points, not a new ABI


def _selected_knobs(module):
    """Knob names in a test module's SELECTIONS dict and in its `knobs` parametrisations."""
    mod = importlib.import_module("tests." + module)
    found = set()
    for sel in getattr(mod, "SELECTIONS", {}).values():
        found |= set(sel)
    for fn in filter(inspect.isfunction, vars(mod).values()):
        for mark in getattr(fn, "pytestmark", []):
            if mark.name == "parametrize" and mark.args[0] == "knobs":
                for case in mark.args[1]:
                    found |= set(case)
    return found


@pytest.mark.parametrize("module,at_least", [("test_edge_parity", {"guard", "bwd_seg", "bwd_parts"}),
                                             ("test_absgrad", {"seg_k", "bwd_union"}),
                                             ("test_alpha_background", {"fwd_parts", "smask", "fwd_part_waves"}),
                                             ("test_camera_grad", {"bwd_prezero", "pbwd_lds_sh"}),
                                             ("test_gpu_parity", {"strip_exact", "fwd_whole_waves"}),
                                             ("test_contrib", set()), ("test_features", set())])
def test_every_knob_the_variant_tests_select_exists(module, at_least):
    found = _selected_knobs(module)
    assert at_least <= found, "the collection no longer sees this module's knobs"
    assert found <= set(_names()), sorted(found - set(_names()))
