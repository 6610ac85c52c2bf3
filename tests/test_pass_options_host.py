"""CPU: the pass with opt-in stages (cm3d_lift_pass_opt, csrc/pass_options.cpp).  The call sequence of every presence combination,
traced over stubs by a stand-alone program built with the address and undefined-behaviour sanitizers (tests/pass_options_sim.cpp) and
compared with the sequence include/cm3d_hip.h states, composed here from the per-stage sequences; the descriptors that make no call;
the rule for the yaw fit's lists inside a pass; and the ctypes layouts of the two new descriptors."""
import ctypes
import itertools
import os
import shutil
import subprocess

import pytest

from tests import pass_options_trace as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMBOS = list(itertools.product((False, True), repeat=4))


def _which(c, f, y, n):
    return ("c" if c else "-") + ("f" if f else "-") + ("y" if y else "-") + ("n" if n else "-")


@pytest.mark.parametrize("waymo", [False, True], ids=["nusc", "waymo"])
def test_every_combination_makes_the_headers_calls_and_ends_at_the_first_error(waymo):
    got = T.group("combo_waymo" if waymo else "combo")
    assert set(got) == {_which(*k) for k in COMBOS}
    for k in COMBOS:
        T.assert_pass(got[_which(*k)], T.composed_sequence(*k, waymo=waymo), _which(*k))


def test_no_option_is_the_plain_pass():
    got = T.traces()
    for name in ("opt.null", "combo.----", "combo_waymo.----"):
        T.assert_pass(got[name], T.plain_sequence(), name)


def test_single_option_passes_are_the_composed_pass_with_one_member():
    got, legacy = T.group("combo"), T.group("legacy")
    assert set(legacy) == {"c---", "-f--", "--y-"}
    for which, trace in legacy.items():
        assert trace == got[which] and trace[0], which


def test_a_bad_descriptor_makes_no_call_wherever_it_stands():
    bad = T.group("bad")
    assert set(bad) == {"opt_size", "opt_size_no_member", "pass_size", "null_pass", "cluster_size", "filter_size", "yaw_size", "nms_size",
                        "nms_size_behind_cluster", "nms_size_alone", "nms_no_thr", "yaw_no_tab_off_behind_filter",
                        "filter_no_on_road_behind_cluster", "cluster_no_cl_idx"}
    for name, trace in bad.items():
        T.assert_refused(trace, name)
    # (cl_idx is an output only of a pass that has index lists)
    T.assert_pass(T.traces()["ok.cluster_without_idx"], T.cluster_sequence(ev=0x50, idx="null", cl_idx="null"), "cluster_without_idx")


def test_yaw_lists_inside_a_pass_are_null_or_what_the_pass_derives():
    rule = T.group("rule")
    for name in ("raw_xyz_behind_cluster", "raw_off_behind_cluster", "raw_pos_behind_filter", "cl_lists_without_cluster"):
        T.assert_refused(rule.pop(name), name)
    T.assert_refused(T.traces()["yaw.own_lists_in_a_pass"], "own_lists_in_a_pass")
    combo = T.group("combo")
    assert set(rule) == {"equal_cfyn", "equal_--yn"}
    for name, trace in rule.items():
        assert trace == combo[name[6:]] and trace[0], name


def test_no_case_writes_to_a_callers_descriptor():
    got = T.traces()
    assert len(got) > 80
    assert not [name for name, (calls, _, _) in got.items() if any("descriptor was changed" in c for c in calls)]


@pytest.mark.parametrize("struct,ctype", [("cm3d_rotated_nms_desc", "RotatedNmsDesc"), ("cm3d_lift_pass_options", "LiftPassOptions")])
def test_descriptor_layouts_match_the_header(tmp_path, struct, ctype):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    from cm3d_amd import _lib
    S = getattr(_lib, ctype)
    names = [n for n, _ in S._fields_]
    assert names == {"RotatedNmsDesc": ["size", "thr", "n_thr", "measure", "class_agnostic", "reserved"],
                     "LiftPassOptions": ["size", "cluster", "filter", "yaw", "nms"]}[ctype]
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cm3d_hip.h"\nint main(void) {\n'
                   + "".join(f'printf("%zu\\n", offsetof({struct}, {n}));\n' for n in names)
                   + f'printf("%zu\\n", sizeof({struct})); return 0; }}\n')
    exe = tmp_path / "t"
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert got == [getattr(S, n).offset for n in names] + [ctypes.sizeof(S)]


def test_new_symbol_within_abi_5_and_unfilled_sizes_never_launch():
    from cm3d_amd import _lib
    L = _lib.lib()
    assert _lib.ABI_VERSION == 5 and L.cm3d_abi_version() == 5
    d, o, n = _lib.LiftPassDesc(), _lib.LiftPassOptions(), _lib.RotatedNmsDesc()
    ref = ctypes.byref
    assert L.cm3d_lift_pass_opt(None, None, None) == -1
    assert L.cm3d_lift_pass_opt(ref(d), None, None) == -1                 # the plain pass refuses the descriptor
    assert L.cm3d_lift_pass_opt(ref(d), ref(o), None) == -1               # options of size 0
    o.size = ctypes.sizeof(o)
    assert L.cm3d_lift_pass_opt(ref(d), ref(o), None) == -1               # no member: the plain pass refuses the descriptor
    o.nms = ctypes.addressof(n)
    d.size = ctypes.sizeof(d)
    assert L.cm3d_lift_pass_opt(ref(d), ref(o), None) == -1               # a member of size 0
    n.size = ctypes.sizeof(n)
    assert L.cm3d_lift_pass_opt(ref(d), ref(o), None) == -1               # no thresholds


def test_pipeline_cpp_does_not_know_the_composed_pass():
    """The plain pass links without pass_options.cpp (tests/lift_pass_sim.cpp's stubs): cm3d_lift_pass and cm3d_pipe_submit are what they
    were; and the box launch is spelled out once per file."""
    csrc = os.path.join(ROOT, "cm3d_amd", "csrc")
    src = open(os.path.join(csrc, "pipeline.cpp")).read()
    assert "lift_pass_opt" not in src and "rotated_nms" not in src and "pass_options" not in src
    assert open(os.path.join(csrc, "pass_options.cpp")).read().count("cm3d_box_nms_bounded(") == 1
    assert open(os.path.join(ROOT, "cm3d_amd", "lifting.py")).read().count("cm3d_box_nms_bounded(") == 1
