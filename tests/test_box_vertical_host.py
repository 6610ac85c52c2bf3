"""CPU: the host statement of the vertical stage (cm3d_amd.boxvertical.box_vertical_host) against the scalar loop of
tests/box_vertical_cases.py to the bit on every list, the overflow case and the apply tables for every quantile pair; closed-form
answers; a second call; kept_box_sizes' composition; the three nuScenes writers and waymo.objects_from_results with the stage's
heights and without; the refusals of the command line; and the geometry case within the bound its own beam table gives."""
import argparse
from types import SimpleNamespace

import numpy as np
import pytest

from cm3d_amd import boxvertical as bv
from tests import box_vertical_cases as vc

CASES = vc.all_cases()


def _host(c, **kw):
    return bv.box_vertical_host(c["xyz"], c["off"], c["idx_cap"], c["box"], c["flags"], c["prior_wlh"], **dict(vc.DEFAULTS, **kw))


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_host_equals_the_scalar_loop(case):
    for run in case["runs"]:
        for qb, qt in vc.QUANTILES:
            kw = dict(vc.DEFAULTS, q_bot=qb, q_top=qt)
            kw.update(run if case["name"] != "apply" else {k: v for k, v in run.items() if k not in ("q_bot", "q_top")})
            got = _host(case, **kw)
            vc.assert_same(got, vc.loop_vertical(case, kw["q_bot"], kw["q_top"], kw["min_points"], kw["lo"], kw["hi"]), (case["name"], kw))
            others = [c for c in range(vc.BOX_STRIDE) if c != 2]
            assert got["box"][:, others].tobytes() == case["box"][:, others].tobytes()


def test_every_status_source_and_route_is_met():
    c = vc.list_case()
    got = _host(c)
    n = np.diff(c["off"])
    assert set(got["vert_status"]) == {0, 1, 2, 4} and set(got["vert_src"]) == {0, 1, 2}
    assert (n <= vc.LANE_MAX).sum() >= 20 and ((n > vc.LANE_MAX) & (n <= vc.LDS_KEYS)).sum() >= 20 and (n > vc.LDS_KEYS).sum() >= 6
    for kind in ("nan", "pinf", "ninf"):
        for where in ("first", "middle", "last"):
            for length in (40, 300):
                assert got["vert_status"][c["names"].index(f"{kind}_{where}{length}")] == 4
    assert got["vert_status"][c["names"].index("nan_last4500")] == 4
    # one multiset in three orders: one answer
    for length in (40, 300):
        rows = [got["vert_z"][c["names"].index(f"{o}{length}")] for o in ("ascending", "descending", "shuffled")]
        assert rows[0].tobytes() == rows[1].tobytes() == rows[2].tobytes()


def test_closed_form_answers():
    prior = np.array([[2.0, 4.0, 2.0]])

    def one(z, qb, qt, **kw):
        xyz = np.zeros((len(z), 4), np.float32)
        xyz[:, 2] = z
        box = np.zeros((1, vc.BOX_STRIDE))
        box[0, 2] = 9.0
        return bv.box_vertical_host(xyz, [0, len(z)], len(z), box, [3], prior, qb, qt, kw.pop("min_points", 1), **kw)
    got = one([3.0, 1.0, 2.0, 0.0, 4.0], 0.0, 1.0, lo=0.5, hi=2.5)
    assert got["vert_z"].tolist() == [[0.0, 4.0]] and got["vert_src"][0] == 1 and got["vert_h"][0] == 4.0 and got["box"][0, 2] == 2.0
    got = one([3.0, 1.0, 2.0, 0.0, 4.0], 0.25, 0.75)                    # ranks 1 and 3: 1.0 and 3.0, extent 2.0 = the prior
    assert got["vert_z"].tolist() == [[1.0, 3.0]] and got["vert_src"][0] == 1 and got["vert_h"][0] == 2.0 and got["box"][0, 2] == 2.0
    got = one([3.0, 1.0, 2.0, 0.0, 4.0], float(np.nextafter(0.25, 0)), float(np.nextafter(0.75, 0)))      # just below: ranks 0 and 2
    assert got["vert_z"].tolist() == [[0.0, 2.0]]
    got = one([3.0, 1.0, 2.0, 0.0, 4.0], 0.5, 0.5)                      # the median twice: extent 0, the prior hung on it
    assert got["vert_z"].tolist() == [[2.0, 2.0]] and got["vert_src"][0] == 2 and got["vert_h"][0] == 2.0 and got["box"][0, 2] == 1.0
    got = one([5.0], 0.0, 1.0)
    assert got["vert_z"].tolist() == [[5.0, 5.0]] and got["box"][0, 2] == 4.0
    got = one([-0.0, 0.0, -0.0, 0.0], 0.0, 1.0)                         # -0.0 sorts before +0.0
    assert np.signbit(got["vert_z"][0]).tolist() == [True, False]
    got = one([0.0, 10.0], 0.0, 1.0)                                    # five priors tall: ground or a wall in the list
    assert got["vert_src"][0] == 0 and got["vert_h"][0] == 2.0 and got["box"][0, 2] == 9.0 and got["vert_entry_z"][0] == 9.0
    got = one([0.0, 1.0], 0.0, 1.0, min_points=3)
    assert got["vert_status"][0] == 1 and got["vert_z"].tolist() == [[0.0, 0.0]] and got["box"][0, 2] == 9.0


def test_the_apply_table_rows():
    c = vc.apply_case()
    for run, want in zip(c["runs"], c["mask0_src"]):
        assert _host(c, **run)["vert_src"][0] == want, run
    got = _host(c, **c["runs"][0])
    row = lambda name: c["names"].index(name)
    src = {name: int(got["vert_src"][row(name)]) for name in c["names"]}
    assert src["both_ends"] == 1 and src["extent_zero"] == 2 and src["top_only"] == 2 and src["too_tall"] == 0
    assert all(src[k] == 0 for k in ("h0_zero", "h0_negative", "h0_nan", "h0_inf", "flags_0", "flags_2", "status_empty", "status_few", "status_not_finite"))
    assert all(src[k] == 1 for k in ("class_below", "class_above", "class_nan", "class_fraction", "entry_nan_source_1"))
    assert [int(got["vert_status"][row(k)]) for k in ("status_empty", "status_few", "status_not_finite")] == [2, 1, 4]
    # an unjudged mask keeps its class's prior height bit for bit, NaN and inf included, and its entry z, whatever that is
    for name, cls in (("h0_zero", 1), ("h0_negative", 2), ("h0_nan", 3), ("h0_inf", 4)):
        assert got["vert_h"][row(name)].tobytes() == c["prior_wlh"][cls, 2].tobytes()
    assert got["vert_h"][row("class_fraction")] == got["vert_z"][row("class_fraction")][1] - got["vert_z"][row("class_fraction")][0]
    for name in ("entry_nan_source_0", "entry_inf_source_0"):
        assert got["box"][row(name), 2].tobytes() == c["box"][row(name), 2].tobytes()
    for name in ("entry_nan_source_1", "entry_inf_source_2"):
        assert np.isfinite(got["box"][row(name), 2]) and got["vert_entry_z"][row(name)].tobytes() == c["box"][row(name), 2].tobytes()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_a_second_call_gives_the_same_box(case):
    first = _host(case, **case["runs"][0])
    again = _host(dict(case, box=first["box"]), **case["runs"][0])
    assert again["box"].tobytes() == first["box"].tobytes() and again["vert_entry_z"].tobytes() == first["box"][:, 2].tobytes()
    for k in ("vert_z", "vert_h", "vert_src", "vert_status"):
        assert again[k].tobytes() == first[k].tobytes(), k


def test_bad_arguments():
    c = vc.apply_case()
    nan, inf = float("nan"), float("inf")
    for kw in (dict(q_bot=-0.1), dict(q_top=1.1), dict(q_bot=0.6, q_top=0.4), dict(q_bot=nan), dict(q_top=nan), dict(min_points=0), dict(lo=0.0),
               dict(lo=nan), dict(hi=inf), dict(hi=nan), dict(lo=1.4, hi=1.3)):
        with pytest.raises(ValueError):
            _host(c, **kw)
        with pytest.raises(ValueError):
            bv.BoxVertical(**kw)
    assert bv.BoxVertical().active and bv.BoxVertical() == bv.BoxVertical(0.02, 0.98, 5, 0.7, 1.3)


# ---------------------------------------------------------------------------------------------------------------- kept_box_sizes
def test_kept_box_sizes_composition():
    import torch
    from cm3d_amd import lifting
    prior = torch.tensor([[2.0, 4.5, 1.7], [0.7, 0.8, 1.75]], dtype=torch.float64)
    flags = torch.tensor([3, 1, 3, 0, 3], dtype=torch.int32)
    box = torch.zeros(5, 10, dtype=torch.float64)
    box[:, 8] = torch.tensor([0.0, 1.0, 1.0, 0.0, 7.0])                  # (the last class lies outside the table: read as 0)
    vert_h = torch.tensor([1.5, 9.0, 1.6, 9.0, 1.9], dtype=torch.float64)
    size_wlh = torch.arange(15, dtype=torch.float64).reshape(5, 3) + 20.0
    with_both = lifting.kept_box_sizes(SimpleNamespace(flags=flags, box=box, vert_h=vert_h, size_wlh=size_wlh, prior_wlh=prior))
    assert with_both.tolist() == [[20.0, 21.0, 1.5], [26.0, 27.0, 1.6], [32.0, 33.0, 1.9]]
    alone = lifting.kept_box_sizes(SimpleNamespace(flags=flags, box=box, vert_h=vert_h, prior_wlh=prior))
    assert alone.tolist() == [[2.0, 4.5, 1.5], [0.7, 0.8, 1.6], [2.0, 4.5, 1.9]]
    today = lifting.kept_box_sizes(SimpleNamespace(flags=flags, box=box, size_wlh=size_wlh))
    assert today.tolist() == size_wlh[[0, 2, 4]].tolist() and size_wlh[0, 2] == 22.0          # (and no buffer was written)


# ---------------------------------------------------------------------------------------------------------------- writers
def _records_heights():
    from tests.test_velocity_host import _records_and_velocities
    rec, vel, tokens, classes = _records_and_velocities()
    rng = np.random.default_rng(28)
    size = classes.prior_wlh[rec[:, 8].astype(int)].copy()
    size[:, 2] = rng.uniform(0.4, 4.0, len(rec))
    size[:3, 2] = [1.55, 1.9000000000000001, 2.5e-5]
    return rec, vel, size, tokens, classes


@pytest.mark.parametrize("with_vel", [True, False])
def test_the_three_writers_agree_on_the_heights(with_vel):
    import json
    from cm3d_amd import lifting
    rec, vel, size, tokens, classes = _records_heights()
    vel = vel if with_vel else None
    meta = {"use_camera": True}
    boxes = lifting.nuscenes_boxes_from_records(rec, tokens, classes, vel=vel, size=size)
    text, n = lifting.nuscenes_results_json(rec, tokens, classes, meta, vel=vel, size=size)
    native = lifting.nuscenes_results_json_native(rec, tokens, classes, meta, vel=vel, size=size)
    assert n == len(rec) and text == json.dumps({"meta": meta, "results": boxes}) and native == text.encode()
    written = sorted(b["size"][2] for bl in boxes.values() for b in bl)
    assert written == sorted(size[:, 2].tolist()) and ('"velocity": [0, 0]' in text) == (not with_vel)
    for bl in boxes.values():
        for b in bl:
            assert b["size"][:2] == [float(x) for x in classes.prior_wlh[classes.names.index(b["detection_name"])][:2]]
    # without the rows: today's bytes
    plain, _ = lifting.nuscenes_results_json(rec, tokens, classes, meta, vel=vel)
    assert plain != text and lifting.nuscenes_results_json_native(rec, tokens, classes, meta, vel=vel) == plain.encode()
    assert lifting.nuscenes_results_json(rec, tokens, classes, meta, vel=vel, size=None)[0] == plain


def test_waymo_objects_with_and_without_the_heights():
    from cm3d_amd import lifting, waymo as wm
    classes = lifting.ClassTable.waymo()
    hb = SimpleNamespace(n_frames=2, mask_off=np.array([0, 3, 5]), class_id=np.array([0, 1, 0, 2, 1]),
                         score=np.array([0.9, 0.8, 0.7, 0.6, 0.5], np.float32))
    rng = np.random.default_rng(3)
    res = dict(box=rng.normal(0, 10, (5, 10)), flags=np.array([3, 3, 1, 3, 0], np.int32))
    meta = [("ctx0", 111), ("ctx1", 222)]
    today = wm.objects_from_results(hb, res, classes, meta)
    vert_h = np.array([1.41, 1.52, 9.0, 1.63, 9.0])
    new = wm.objects_from_results(hb, dict(res, vert_h=vert_h), classes, meta)
    a, b = wm.decode_objects(wm.encode_objects(today)), wm.decode_objects(wm.encode_objects(new))
    assert [o["height"] for o in a] == [float(classes.prior_wlh[c, 2]) for c in (0, 1, 2)]
    assert [o["height"] for o in b] == [1.41, 1.52, 1.63]
    for x, y in zip(a, b):
        assert {k: v for k, v in x.items() if k != "height"} == {k: v for k, v in y.items() if k != "height"}
    # the prior's heights given as vert_h: today's bytes
    same = wm.objects_from_results(hb, dict(res, vert_h=classes.prior_wlh[hb.class_id, 2]), classes, meta)
    assert wm.encode_objects(same) == wm.encode_objects(today)


def test_waymo_records_writer_takes_the_heights():
    from cm3d_amd import lifting, pipeline_waymo as pw, waymo as wm
    classes = lifting.ClassTable.waymo()
    rec = np.zeros((3, 10))
    rec[:, 8], rec[:, 7] = [0, 1, 2], [0.9, 0.8, 0.7]
    rec[:, lifting.REC_FRAME_A], rec[:, lifting.REC_FRAME_B] = 0, [1, 0, 1]
    meta = {(0, 0): ("c", 5), (0, 1): ("c", 6)}
    today = wm.decode_objects(wm.encode_objects(pw.objects_from_records(rec, ["s"], "", classes, meta)))
    new = wm.decode_objects(wm.encode_objects(pw.objects_from_records(rec, ["s"], "", classes, meta, height=[1.1, 1.2, 1.3])))
    assert [o["height"] for o in today] == [float(classes.prior_wlh[c, 2]) for c in (1, 0, 2)]        # (frame 0 first)
    assert [o["height"] for o in new] == [1.2, 1.1, 1.3] and [o["width"] for o in new] == [o["width"] for o in today]
    with pytest.raises(ValueError):
        pw.objects_from_records(rec, ["s"], "", classes, meta, height=[1.0])


# ---------------------------------------------------------------------------------------------------------------- command line
def _parser():
    ap = argparse.ArgumentParser()
    bv.add_arguments(ap)
    return ap


def test_command_line_refusals():
    ap = _parser()
    assert bv.from_args(ap.parse_args([])) is None and bv.from_args(ap.parse_args(["--vertical", "medoid"])) is None
    assert bv.from_args(ap.parse_args(["--vertical", "fit"])) == bv.BoxVertical()
    got = bv.from_args(ap.parse_args(["--vertical", "fit", "--vertical-quantiles", "0.05,0.9", "--vertical-min-points", "8", "--vertical-ratio", "0.6,1.4"]))
    assert got == bv.BoxVertical(0.05, 0.9, 8, 0.6, 1.4)
    refused = [["--vertical-quantiles", "0.1,0.9"], ["--vertical-min-points", "3"], ["--vertical-ratio", "0.7,1.3"],
               ["--vertical", "medoid", "--vertical-min-points", "3"], ["--vertical", "fit", "--vertical-quantiles", "0.5"],
               ["--vertical", "fit", "--vertical-quantiles", "0.9,0.1"], ["--vertical", "fit", "--vertical-quantiles", "0.1,1.5"],
               ["--vertical", "fit", "--vertical-quantiles", "a,b"], ["--vertical", "fit", "--vertical-min-points", "0"],
               ["--vertical", "fit", "--vertical-ratio", "1.3,0.7"], ["--vertical", "fit", "--vertical-ratio", "0,1.3"],
               ["--vertical", "fit", "--vertical-ratio", "0.7,inf"], ["--vertical", "fit", "--vertical-ratio", "0.7"]]
    for argv in refused:
        with pytest.raises(ValueError):
            bv.from_args(ap.parse_args(argv))
        with pytest.raises(SystemExit):
            bv.from_args(ap.parse_args(argv), ap)
    with pytest.raises(SystemExit):
        ap.parse_args(["--vertical", "top"])
    assert "untuned" in ap.format_help().lower()


def test_the_entry_points_refuse_before_any_work():
    from cm3d_amd import pipeline_kitti, pipeline_nuscenes, pipeline_waymo
    for main in (pipeline_nuscenes.main, pipeline_waymo.main):
        for argv in (["--vertical-min-points", "3"], ["--vertical", "medoid", "--vertical-ratio", "0.7,1.3"],
                     ["--vertical", "fit", "--vertical-quantiles", "0.9,0.1"]):
            with pytest.raises(SystemExit) as e:
                main(argv)
            assert e.value.code == 2, argv
    with pytest.raises(SystemExit) as e:                                 # KITTI does not take the flags
        pipeline_kitti.main(["--vertical", "fit"])
    assert e.value.code == 2


# ---------------------------------------------------------------------------------------------------------------- geometry
@pytest.mark.parametrize("d,visible_from", vc.GEO_SCENES)
def test_geometry_within_the_bound_of_the_beam_table(d, visible_from):
    s = vc.geometry_scene(d, visible_from)
    box = np.zeros((1, vc.BOX_STRIDE))
    box[0, 2] = vc.medoid_z(s["xyz"])
    got = bv.box_vertical_host(s["xyz"], [0, s["n"]], s["n"], box, [3], [[2.1, 4.9, vc.GEO_PRIOR_H]], **vc.DEFAULTS)
    src, h, z = int(got["vert_src"][0]), float(got["vert_h"][0]), float(got["box"][0, 2])
    print(f"range {d} m, visible from {visible_from} m: {s['n']} points, beam gap {s['dz']:.3f} m, source {src}: h {h:.3f} (true {s['true_h']}), "
          f"z {z:.3f} (true {s['true_z']}; the medoid's z {box[0, 2]:.3f}), bounds {s['bound'].get(src)}")
    assert got["vert_status"][0] == 0 and src in s["sources"]
    assert abs(h - s["true_h"]) <= s["bound"][src]["h"] and abs(z - s["true_z"]) <= s["bound"][src]["z"]
