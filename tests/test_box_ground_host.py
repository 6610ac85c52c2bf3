"""CPU: the host statement of the ground stage (cm3d_amd.boxground.box_ground_host) against the scalar loop of tests/box_ground_cases.py
on every case and run, to the bit; what the cases are built for; BoxGround's validation and the flags' errors; and a geometry case within
a derived bound."""
import argparse
import math

import numpy as np
import pytest

from cm3d_amd import boxground as bg
from tests import box_ground_cases as gc

CASES = gc.all_cases()
IDS = [c["name"] for c in CASES]


@pytest.fixture(scope="module")
def clouds(oracle):
    return {c["name"]: gc.cloud(oracle, c) for c in CASES}


def _host(case, cloud, run):
    return bg.box_ground_host(cloud[0], cloud[1], case["mask_off"], case["box"], case["flags"], case["prior_wlh"], zref=case["zref"],
                              vert=case["vert"], **gc.params(run))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_host_statement_equals_the_scalar_loop(case, clouds):
    cloud = clouds[case["name"]]
    others = [c for c in range(gc.BOX_STRIDE) if c != 2]
    for run in case["runs"]:
        exp = gc.loop_ground(case, cloud[0], cloud[1], **gc.params(run))
        got = _host(case, cloud, run)
        gc.assert_same(got, exp, (case["name"], run))
        assert got["box"][:, others].tobytes() == case["box"][:, others].tobytes()
        keep = got["ground_src"] == 0
        assert got["box"][keep, 2].tobytes() == case["box"][keep, 2].tobytes()


def test_the_defaults_are_the_issues():
    assert gc.DEFAULTS == bg.BoxGround().params() and gc.BINS == 128 and gc.DZ == 11.0 / 256.0
    assert bg.RESULTS == ("ground_z", "ground_n", "ground_h", "ground_src", "ground_status", "ground_zref")


@pytest.mark.parametrize("with_vert", [True, False])
def test_the_edge_cases_sit_on_their_edges(with_vert, clouds):
    """Status and n of every named mask, and the bin of those built for one, at the defaults; then what the other runs move."""
    c = next(k for k in CASES if k["name"] == ("edges" if with_vert else "edges_no_vertical"))
    cloud = clouds[c["name"]]
    got = _host(c, cloud, {})
    at = {n: i for i, n in enumerate(c["names"])}
    for n, i in at.items():
        assert (got["ground_status"][i], got["ground_n"][i]) == c["expect"].get(n, (0, 25)), n
    for n, b in c["bins"].items():
        assert got["ground_z"][at[n]] == 1.0 - 5.0 + (b + 0.5) * gc.DZ, n
    assert (got["ground_z"][got["ground_status"] != 0] == 0.0).all()
    assert {0, 1, 2, 4} <= set(got["ground_status"])
    assert got["ground_src"][at["flags_0"]] == 0 and got["ground_src"][at["flags_2"]] == 0 and got["ground_src"][at["class_fraction"]] > 0
    # the out-of-range classes are read as class 0, the fraction as class 1
    for n in ("class_below", "class_above", "class_nan"):
        assert got["ground_src"][at[n]] == (1 if with_vert else 2), n         # (with a top of 1.2: 0.75 heights of class 0 over the ground)
        assert with_vert or got["ground_h"][at[n]] == c["prior_wlh"][0, 2], n
    if with_vert:
        assert got["ground_h"][at["flags_0"]] == c["vert"]["vert_h"][at["flags_0"]]           # unjudged: what the vertical stage left
        assert got["ground_zref"].tobytes() == c["zref"].tobytes()
    else:
        assert got["ground_h"][at["flags_0"]] == c["prior_wlh"][0, 2]
        assert got["ground_zref"].tobytes() == c["box"][:, 2].tobytes()
    # min_points 21: the mask of 20 members falls to status 1; quantile 1: the last occupied bin; a radius one float32 below 3: the
    # points on the circle are out
    runs = {tuple(sorted(r.items())): _host(c, cloud, r) for r in c["runs"]}
    assert runs[(("min_points", 21),)]["ground_status"][at["enough_20"]] == 1
    assert runs[(("quantile", 1.0),)]["ground_z"][at["window"]] == 1.0 - 5.0 + 127.5 * gc.DZ
    assert runs[(("quantile", 0.0),)]["ground_z"][at["k_first_of_next"]] == 1.0 - 5.0 + 80.5 * gc.DZ
    assert runs[(("radius", gc._dn(3.0)),)]["ground_n"][at["on_circle"]] == 0


@pytest.mark.parametrize("with_vert", [True, False])
def test_the_apply_table_takes_every_branch(with_vert, clouds):
    c = next(k for k in CASES if k["name"] == ("apply" if with_vert else "apply_no_vertical"))
    cloud = clouds[c["name"]]
    got = _host(c, cloud, {})
    g = c["g"]
    for i, n in enumerate(c["names"]):
        assert got["ground_src"][i] == c["src"][n], n
        h0 = c["prior_wlh"][int(c["box"][i, 8]), 2]
        if n != "few_members":
            assert got["ground_z"][i] == g
        if got["ground_src"][i] == 1:
            top = c["vert"]["vert_z"][i, 1]
            assert got["ground_h"][i] == top - g and got["box"][i, 2] == g + (top - g) * 0.5
        elif got["ground_src"][i] == 2:
            assert got["ground_h"][i] == h0 and got["box"][i, 2] == g + h0 * 0.5
        else:
            was = c["vert"]["vert_h"][i] if with_vert else h0
            assert np.array([got["ground_h"][i]]).tobytes() == np.array([was]).tobytes() and got["box"][i, 2] == c["box"][i, 2]
    assert [int(_host(c, cloud, r)["ground_src"][0]) for r in c["runs"][:8]] == c["mask0_src"]
    assert set(c["src"].values()) == ({0, 1, 2} if with_vert else {0, 2})


def test_the_many_cases_cross_the_launchs_own_chunk_twice():
    """The chunk is the launch's, from the batch's shape (cm3d_box_ground_chunk, host code): the smallest, one in between and the
    largest are each crossed at least twice by the frame of 130 masks; from 33 on every wave scans and a wave scans several masks."""
    from cm3d_amd import _lib
    L = _lib.lib()
    for name, _, _, chunk in gc.MANY_SHAPES:
        c = next(k for k in CASES if k["name"] == name)
        per_frame = np.diff(c["mask_off"])
        assert int(L.cm3d_box_ground_chunk(len(per_frame), int(per_frame.max()))) == chunk, name
        assert per_frame.max() == 130 and per_frame.max() > 2 * chunk and sorted(per_frame)[-2] == 70 > chunk and len(c["sweeps"]) == 4
    assert gc.MANY_SHAPES[0][3] == 8 and gc.MANY_SHAPES[-1][3] == gc.CHUNK and 16 < gc.MANY_SHAPES[1][3] < gc.CHUNK
    # told 20 masks per frame at most, the launch of the 128-frame shape takes chunks of 10: a workgroup then walks the frame of 130
    assert int(L.cm3d_box_ground_chunk(128, 20)) == 10
    c = CASES[4]
    assert not np.array_equal(c["sweeps"][0][1], c["sweeps"][1][1]) and max(np.diff(c["sweep_row_off"][c["frame_sweep_off"]])) <= 2048


def test_box_ground_validation():
    assert bg.BoxGround().params() == gc.DEFAULTS and bg.BoxGround().active
    g = bg.BoxGround(radius="2", quantile=0, min_points=3.0, down=1, up=0, lo=1, hi=1)
    assert (g.radius, g.quantile, g.min_points, g.down, g.up, g.lo, g.hi) == (2.0, 0.0, 3, 1.0, 0.0, 1.0, 1.0) and isinstance(g.min_points, int)
    nan, inf = float("nan"), float("inf")
    bad = [dict(radius=0.0), dict(radius=-1.0), dict(radius=nan), dict(radius=inf), dict(quantile=-0.01), dict(quantile=1.01), dict(quantile=nan),
           dict(min_points=0), dict(down=0.0), dict(down=-1.0), dict(down=nan), dict(down=inf), dict(up=-0.1), dict(up=nan), dict(up=inf),
           dict(lo=0.0), dict(lo=nan), dict(hi=nan), dict(hi=inf), dict(lo=1.3, hi=0.7)]
    for kw in bad:
        with pytest.raises(ValueError):
            bg.BoxGround(**kw)
        with pytest.raises(ValueError):
            bg.box_ground_host(np.zeros((0, 4), np.float32), [0, 0], [0, 0], np.zeros((0, 10)), [], gc.PRIOR, **kw)
    with pytest.raises(ValueError):
        bg.box_ground_host(np.zeros((0, 4), np.float32), [0, 0], [0, 0, 0], np.zeros((0, 10)), [], gc.PRIOR)
    none = bg.box_ground_host(np.zeros((0, 4), np.float32), [0, 0], [0, 0], np.zeros((0, 10)), [], gc.PRIOR)
    assert all(len(none[k]) == 0 for k in bg.RESULTS)


def _parse(argv):
    ap = argparse.ArgumentParser()
    bg.add_arguments(ap)
    return ap, ap.parse_args(argv)


def test_the_flags():
    ap, args = _parse([])
    assert bg.from_args(args, ap) is None
    ap, args = _parse(["--ground", "medoid"])
    assert bg.from_args(args, ap) is None
    ap, args = _parse(["--ground", "fit"])
    assert bg.from_args(args, ap).params() == gc.DEFAULTS
    ap, args = _parse(["--ground", "fit", "--ground-radius", "2.5", "--ground-quantile", "0.2", "--ground-min-points", "7", "--ground-window",
                       "3,0.25", "--ground-ratio", "0.5,1.5"])
    assert bg.from_args(args, ap).params() == dict(radius=2.5, quantile=0.2, min_points=7, down=3.0, up=0.25, lo=0.5, hi=1.5)
    for flag, value in (("--ground-radius", "2"), ("--ground-quantile", "0.2"), ("--ground-min-points", "3"), ("--ground-window", "3,1"),
                        ("--ground-ratio", "0.5,1.5")):
        for mode in ([], ["--ground", "medoid"]):
            ap, args = _parse(mode + [flag, value])
            with pytest.raises(ValueError, match="needs --ground fit"):
                bg.from_args(args)
            with pytest.raises(SystemExit):
                bg.from_args(args, ap)
    for argv in (["--ground-window", "3"], ["--ground-window", "3,1,2"], ["--ground-ratio", "a,b"], ["--ground-radius", "-1"],
                 ["--ground-quantile", "2"], ["--ground-window", "0,1"], ["--ground-ratio", "2,1"], ["--ground-min-points", "0"]):
        ap, args = _parse(["--ground", "fit"] + argv)
        with pytest.raises(ValueError):
            bg.from_args(args)
        with pytest.raises(SystemExit):
            bg.from_args(args, ap)
    with pytest.raises(SystemExit):
        _parse(["--ground", "plane"])


# ------------------------------------------------------------------------------------------------ geometry
SENSOR_H, BEAMS, AZIMUTHS = 1.84, np.deg2rad(np.linspace(-30.67, 10.67, 32)), 1800


def _scene(slope, direction, obj_range=11.0):
    """A spinning LiDAR 1.84 m above a plane z = gx x + gy y of slope `slope` (|gradient|) rising along `direction`, noise-free, and an
    upright object 2 m wide and 1.6 m tall whose near face stands at obj_range along x: its face's points (12 columns, the beams that
    hit it) replace the ground returns behind it.  Returns (points float32, centre of the box, the medoid's z)."""
    gx, gy = slope * math.cos(direction), slope * math.sin(direction)
    az = np.linspace(-np.pi, np.pi, AZIMUTHS, endpoint=False)
    e, a = np.meshgrid(BEAMS, az, indexing="ij")
    denom = gx * np.cos(e) * np.cos(a) + gy * np.cos(e) * np.sin(a) - np.sin(e)
    with np.errstate(divide="ignore"):
        r = np.where(denom > 1e-3, SENSOR_H / denom, np.inf)
    ok = (r < 60.0).reshape(-1)
    with np.errstate(invalid="ignore"):
        ground = np.stack([(r * np.cos(e) * np.cos(a)).reshape(-1), (r * np.cos(e) * np.sin(a)).reshape(-1), (SENSOR_H + r * np.sin(e)).reshape(-1)], 1)[ok]
    shadow = (ground[:, 0] > obj_range) & (np.abs(ground[:, 1]) < 1.0 * ground[:, 0] / obj_range)
    ground = ground[~shadow]
    base = gx * obj_range                            # the plane under the face's middle
    zs = SENSOR_H + obj_range * np.tan(BEAMS)
    zs = zs[(zs > base + 0.15) & (zs < base + 1.6)]          # (above the plane at every y of the face: |gy| <= 0.1)
    face = np.array([[obj_range, y, z] for z in zs for y in np.linspace(-1.0, 1.0, 12)])
    pts = np.concatenate([ground, face], 0).astype(np.float32)
    d = np.sqrt(((face[:, None] - face[None]) ** 2).sum(-1)).sum(1)
    return pts, (obj_range + 1.0, 0.0), float(np.float32(face[np.argmin(d), 2])), len(face), (gx, gy)


@pytest.mark.parametrize("slope", [0.0, 0.03, 0.1])
@pytest.mark.parametrize("direction", [0.0, 2.0, -2.6])
def test_geometry_ground_under_an_object_on_a_slope(slope, direction):
    """Bound.  Every member lies inside the circle of radius R around c, so a ground member's height is plane(c) + gradient . (p - c),
    within s R of plane(c); an object point stands above the plane at its own x, y, so it is not below plane(c) - s R either.  Let the
    members hold n_o object points and n_g ground points.  k = (int)(Q (n - 1)) <= Q n; with n_o / n < 1 - Q (asserted) n_g > Q n >= k,
    so at least k + 1 members are ground and the value of rank k is no higher than the highest ground member: it lies in
    [plane(c) - s R, plane(c) + s R].  The whole of that range lies inside the window around the medoid's z (asserted), so the window
    cuts no ground member off.  ground_z is the centre of the bin that holds that value: within dz / 2 of it.  The coordinates are
    float32: a height is off by half an ulp, and a point up to an ulp outside the circle may count as inside -- a few ulps of the
    largest coordinate cover both.  So |ground_z - plane(c)| <= s R + dz / 2 + 4 ulp.  Derived, not tuned."""
    pts, c, zref, n_face, (gx, gy) = _scene(slope, direction)
    R, Q = gc.DEFAULTS["radius"], gc.DEFAULTS["quantile"]
    box = np.zeros((1, gc.BOX_STRIDE))
    box[0, 0], box[0, 1], box[0, 2], box[0, 8] = c[0], c[1], zref, 0.0
    got = bg.box_ground_host(pts, [0, len(pts)], [0, 1], box, [3], gc.PRIOR)
    plane_c = gx * c[0] + gy * c[1]
    n = int(got["ground_n"][0])
    p64 = pts.astype(np.float64)
    t = (p64[:, 2] - (zref - gc.DEFAULTS["down"])) / gc.DZ
    inside = ((p64[:, 0] - c[0]) ** 2 + (p64[:, 1] - c[1]) ** 2 <= R * R) & (t >= 0.0) & (t < 128.0)
    n_obj = int(inside[-n_face:].sum())
    assert got["ground_status"][0] == 0 and n == int(inside.sum()) and n_obj > 0
    assert n_obj / n < 1.0 - Q, (n_obj, n)
    assert zref - gc.DEFAULTS["down"] < plane_c - slope * R and plane_c + slope * R < zref + gc.DEFAULTS["up"]
    bound = slope * R + gc.DZ / 2 + 4 * float(np.spacing(np.float32(np.abs(pts).max())))
    err = abs(float(got["ground_z"][0]) - plane_c)
    print(f"slope {slope} towards {direction}: {n} members, {n_obj} of the object; ground_z off by {err:.4f} m (bound {bound:.4f}); the medoid "
          f"stands {zref - plane_c:.2f} m above the plane")
    assert err <= bound
    # the prior stood on that ground: the box's bottom is the ground
    assert got["ground_src"][0] == 2 and got["box"][0, 2] - gc.PRIOR[0, 2] * 0.5 == pytest.approx(got["ground_z"][0], abs=1e-12)
