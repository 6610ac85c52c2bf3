"""CPU: the host statement of the box velocity stage (cm3d_amd.velocity.track_velocity_host, the rule of include/cm3d_hip.h's
cm3d_box_velocity) against a separately written plain loop, scipy's assignment totals and closed-form answers on tests/velocity_cases.py;
and the three nuScenes writers given velocities.  Where equal-weight assignments tie, only the written tie rule is asserted (against
the plain loop and the pinned answers); nothing is claimed about scipy's choice, only about its total, which is unique."""
import json
import math

import numpy as np
import pytest

from cm3d_amd import velocity as V
from tests import velocity_cases as vc

KMAX = 1000000
CASES = vc.all_cases()
IDS = [c["name"] for c in CASES]


# ------------------------------------------------------------------------------------------------ the plain loop
def _plain_assign(W, n, m):
    """Hungarian method with potentials, scalar, rows 1..n <= columns 1..m; ties: the least reduced cost, then an unassigned
    column, then the lowest column.  Returns p: the row of every column (0: none)."""
    INF = 1 << 30
    u, v, p, way = [0] * (n + 1), [0] * (m + 1), [0] * (m + 1), [0] * (m + 1)
    for i in range(1, n + 1):
        p[0] = i
        minv, used, j0 = [INF] * (m + 1), [False] * (m + 1), 0
        while True:
            used[j0] = True
            i0, best, j1 = p[j0], None, 0
            row = W[i0 - 1]
            for j in range(1, m + 1):
                if used[j]:
                    continue
                cur = KMAX - row[j - 1] - u[i0] - v[j]
                if cur < minv[j]:
                    minv[j], way[j] = cur, j0
                key = (minv[j], p[j] != 0, j)
                if best is None or key < best:
                    best, j1 = key, j
            delta = best[0]
            for j in range(m + 1):
                if used[j]:
                    u[p[j]] += delta
                    v[j] -= delta
                else:
                    minv[j] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while j0:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
    return p


def _plain(box, flags, mask_off, class_id, frame_next, frame_time, track_group, max_speed, max_dt):
    box, F, M = box.tolist(), len(mask_off) - 1, len(flags)
    flags, mask_off, class_id, frame_next = flags.tolist(), mask_off.tolist(), class_id.tolist(), frame_next.tolist()
    frame_time, track_group, max_speed = frame_time.tolist(), track_group.tolist(), max_speed.tolist()
    nxt, prv, status, totals = [-1] * M, [-1] * M, 0, {}
    for f in range(F):
        n = frame_next[f]
        if n < -1 or n >= F:
            status |= 1
            continue
        if n < 0:
            continue
        dt = frame_time[n] - frame_time[f]
        if not 0.0 < dt <= max_dt:
            continue
        f0, n0 = mask_off[f], mask_off[n]
        P, G = mask_off[f + 1] - f0, mask_off[n + 1] - n0
        if P > 1024 or G > 1024:                   # CM3D_MAX_MASKS_PER_FRAME: the solver's capacity; no link, status bit 1
            status |= 2
            continue
        W = [[0] * G for _ in range(P)]
        for a in range(P):
            for b in range(G):
                i, j = f0 + a, n0 + b
                if flags[i] & 3 != 3 or flags[j] & 3 != 3 or track_group[class_id[i]] != track_group[class_id[j]]:
                    continue
                dx, dy = box[j][0] - box[i][0], box[j][1] - box[i][1]
                d2 = dx * dx + dy * dy
                gate = max_speed[track_group[class_id[i]]] * dt
                if d2 <= gate * gate:
                    W[a][b] = 1 + int((1.0 - math.sqrt(d2) / gate) * float(KMAX - 1))
        totals[f] = 0
        if P == 0 or G == 0:
            continue
        if P <= G:
            p = _plain_assign(W, P, G)
            pairs = [(p[c] - 1, c - 1) for c in range(1, G + 1) if p[c]]
        else:
            Wt = [[W[a][b] for a in range(P)] for b in range(G)]
            p = _plain_assign(Wt, G, P)
            pairs = [(c - 1, p[c] - 1) for c in range(1, P + 1) if p[c]]
        for a, b in pairs:
            if W[a][b] > 0:
                nxt[f0 + a], prv[n0 + b] = n0 + b, f0 + a
                totals[f] += W[a][b]
    frame_of = [f for f in range(F) for _ in range(mask_off[f + 1] - mask_off[f])]
    vel, src = [[0.0, 0.0] for _ in range(M)], [0] * M
    for i in range(M):
        if flags[i] & 3 != 3:
            continue
        t, a, b = frame_time[frame_of[i]], nxt[i], prv[i]
        if a >= 0 and b >= 0 and frame_time[frame_of[a]] - frame_time[frame_of[b]] <= max_dt:
            span, hi, lo, src[i] = frame_time[frame_of[a]] - frame_time[frame_of[b]], box[a], box[b], 3
        elif a >= 0 and frame_time[frame_of[a]] - t <= max_dt:
            span, hi, lo, src[i] = frame_time[frame_of[a]] - t, box[a], box[i], 1
        elif b >= 0 and t - frame_time[frame_of[b]] <= max_dt:
            span, hi, lo, src[i] = t - frame_time[frame_of[b]], box[i], box[b], 2
        else:
            continue
        vel[i] = [(hi[0] - lo[0]) / span, (hi[1] - lo[1]) / span]
    return dict(next_match=nxt, prev_match=prv, vel=vel, vel_src=src, status=status), totals


@pytest.fixture(scope="module")
def host():
    return {c["name"]: V.track_velocity_host(*vc.args_of(c), want_weights=True) for c in CASES}


def _total(case, res, f):
    W = res["weights"][f]
    f0, n0 = int(case["mask_off"][f]), int(case["mask_off"][case["frame_next"][f]])
    nm = res["next_match"][f0:f0 + W.shape[0]]
    rows = np.flatnonzero(nm >= 0)
    return int(W[rows, nm[rows] - n0].sum())


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_host_statement_equals_the_plain_loop(case, host):
    got = host[case["name"]]
    exp, totals = _plain(*vc.args_of(case))
    for k in ("next_match", "prev_match", "vel_src"):
        assert np.array_equal(got[k], np.asarray(exp[k], np.int32)), k
    assert np.asarray(exp["vel"], np.float64).reshape(-1, 2).tobytes() == got["vel"].tobytes()
    assert got["status"] == exp["status"]
    for f, W in got["weights"].items():
        assert _total(case, got, f) == totals[f]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_total_weight_is_the_maximum(case, host):
    from scipy.optimize import linear_sum_assignment
    res = host[case["name"]]
    for f, W in res["weights"].items():
        r, c = linear_sum_assignment(W, maximize=True)
        assert _total(case, res, f) == int(W[r, c].sum()), f
    # one to one, both directions agree
    nm, pm = res["next_match"], res["prev_match"]
    ids = np.flatnonzero(nm >= 0)
    assert len(set(nm[ids].tolist())) == ids.size and np.array_equal(pm[nm[ids]], ids) and (pm >= 0).sum() == ids.size


@pytest.mark.parametrize("case", [c for c in CASES if c["expect"]], ids=[c["name"] for c in CASES if c["expect"]])
def test_pinned_answers(case, host):
    res = host[case["name"]]
    for k, e in case["expect"].items():
        if k == "weights":
            for f, w in e.items():
                assert np.array_equal(res["weights"][f], np.asarray(w)), (k, f)
        elif k == "status":
            assert res["status"] == e
        elif k == "vel":
            assert np.asarray(e, np.float64).reshape(-1, 2).tobytes() == res["vel"].tobytes()          # exact: dyadic inputs
        else:
            assert np.array_equal(res[k], np.asarray(e)), k


def test_every_family_is_exercised(host):
    """The cases cannot rot into trivial ones: links are refused for each reason, every solver instance and both weight sources get
    a link, both orientations occur, every vel_src value appears."""
    sizes = [(W.shape, int((W > 0).sum())) for r in host.values() for W in r["weights"].values()]
    big = [max(s) for s, _ in sizes]
    assert any(b <= 64 for b in big) and any(64 < b <= 128 for b in big) and any(128 < b <= 256 for b in big) and any(b > 256 for b in big)
    assert any(s[0] * s[1] == 8192 for s, _ in sizes) and any(s[0] * s[1] == 8256 for s, _ in sizes)
    assert any(s[0] > s[1] for s, _ in sizes) and any(s[0] < s[1] for s, _ in sizes)
    assert (1024, 300) in [s for s, _ in sizes] and all(npos > 0 for s, npos in sizes if min(s) >= 63)
    assert {0, 1, 2, 3} <= set(np.concatenate([r["vel_src"] for r in host.values()]).tolist())
    assert host["frame_next_out_of_range_7"]["status"] == 1 and host["two_scenes"]["status"] == 0
    assert 0 not in host["dt_one_ulp_above_max_dt"]["weights"] and 0 in host["dt_exactly_max_dt"]["weights"]


def test_a_frame_beyond_the_capacity_takes_its_link_out_and_no_other(host):
    """1025 masks on either side of a link: status bit 1, the slot holds no pair, none of its masks gets a match or a velocity; the
    third scene's link of 5 x 4 masks is the one of the same batch without the two scenes in front."""
    from cm3d_amd import _lib
    case, res = vc.by_name("over_capacity"), host["over_capacity"]
    assert max(max(c) for c in vc.OVER_CAPACITY_COUNTS) == _lib.MAX_MASKS_PER_FRAME + 1
    off = case["mask_off"]
    assert np.diff(off).tolist() == [n for pair in vc.OVER_CAPACITY_COUNTS for n in pair]
    assert res["status"] == 2 and res["pair_off"].tolist() == [0, 0, 0, 0, 0, 20, 20] and list(res["weights"]) == [4]
    m4 = int(off[4])
    for k in ("next_match", "prev_match"):
        assert (res[k][:m4] == -1).all(), k
    assert not res["vel_src"][:m4].any() and not res["vel"][:m4].any()
    assert (res["next_match"][m4:] >= 0).sum() == 3 and (res["next_match"][m4:][res["next_match"][m4:] >= 0] >= off[5]).all()
    alone = dict(case, box=case["box"][m4:], flags=case["flags"][m4:], class_id=case["class_id"][m4:], mask_off=off[4:] - m4,
                 frame_next=np.array([1, -1], np.int32), frame_time=case["frame_time"][4:])
    lone = V.track_velocity_host(*vc.args_of(alone))
    assert lone["status"] == 0 and np.array_equal(np.where(lone["next_match"] >= 0, lone["next_match"] + m4, -1), res["next_match"][m4:])
    assert lone["vel"].tobytes() == res["vel"][m4:].tobytes() and np.array_equal(lone["vel_src"], res["vel_src"][m4:])


@pytest.mark.parametrize("pair", vc.clamp_cases(), ids=[c["name"] for c, _ in vc.clamp_cases()])
def test_mask_off_is_read_clamped(pair):
    """A mask_off entry outside [0, M] is read as the nearest bound: the statement on the raw offsets is the statement on the clamped
    ones, byte for byte."""
    raw, clamped = pair
    M = len(raw["flags"])
    assert not np.array_equal(raw["mask_off"], clamped["mask_off"])
    assert np.array_equal(np.clip(raw["mask_off"], 0, M), clamped["mask_off"]) and (np.diff(clamped["mask_off"]) >= 0).all()
    a, b = V.track_velocity_host(*vc.args_of(raw)), V.track_velocity_host(*vc.args_of(clamped))
    for k in ("next_match", "prev_match", "vel_src", "vel", "pair_off"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["status"] == b["status"] == 0 and (a["next_match"] >= 0).sum() == 4


def test_the_greedy_case_differs_from_greedy(host):
    case = vc.by_name("mutual_nearest_neighbours")
    res = host[case["name"]]
    W = res["weights"][0]
    assert W[1, 0] == W.max()                                   # b and c: each other's nearest neighbour
    assert vc.greedy_total(W) < _total(case, res, 0)
    assert res["next_match"][1] != 2                            # ... and the optimum separates them


def test_frame_times_subtract_integers():
    ts = np.array([1533151603547590, 1533151604048025, 1533151604548459], np.int64)
    t = V.frame_times(ts)
    assert t.tolist() == [0.0, 500435 * 1e-6, 1000869 * 1e-6]
    assert V.frame_next_of(["a", "b", "c"], ["b", "c", ""]).tolist() == [1, 2, -1]
    assert V.frame_next_of(["a", "b"], ["b", "z"]).tolist() == [1, -1]


def test_velocity_switches():
    from cm3d_amd.lifting import ClassTable
    ct = ClassTable.nuscenes()
    sp = V.Velocity().speed_by_group(ct)
    assert sp[ct.index("car")] == 40.0 and sp[ct.index("bicycle")] == 15.0 and sp[ct.index("pedestrian")] == 5.0
    assert sp[ct.index("barrier")] == 1.0 and sp[ct.index("traffic_cone")] == 1.0
    assert V.Velocity({"car": 25.0}).speed_by_group(ct)[ct.index("car")] == 25.0
    assert V.parse_max_speed("car=30, pedestrian=3.5") == {"car": 30.0, "pedestrian": 3.5}
    with pytest.raises(ValueError):
        V.Velocity(max_dt=0.0)
    with pytest.raises(ValueError):
        V.Velocity({"car": float("nan")})


# ------------------------------------------------------------------------------------------------ the writers, given velocities
def _records_and_velocities():
    from cm3d_amd import lifting
    classes = lifting.ClassTable.nuscenes()
    rng = np.random.default_rng(19)
    tokens = [f"tok{i:02d}" for i in range(7)]                                   # token 3 gets no box
    k = 40
    rec = np.zeros((k, 10), np.float64)
    rec[:, :3] = rng.uniform(-2000, 2000, (k, 3))
    ang = rng.uniform(-np.pi, np.pi, k)
    rec[:, 3], rec[:, 4] = np.cos(ang / 2), np.sin(ang / 2)
    rec[:, 5] = np.sort(rng.choice([0, 1, 2, 4, 5, 6], k))
    rec[:, 7], rec[:, 8], rec[:, 9] = rng.uniform(0, 1, k), rng.integers(0, len(classes.names), k), 3
    vel = rng.uniform(-30, 30, (k, 2))
    vel[:10] = [[0.0, 0.0], [-0.0, 0.0], [3.0, -4.0], [1e-7, 2.5e-5], [1e22, -1e16], [np.inf, 1.0], [-np.inf, np.nan], [0.1, 0.2],
                [123456789.125, 1e15], [5e-324, 1.7976931348623157e308]]
    return rec, vel, tokens, classes


def test_writers_agree_given_velocities():
    from cm3d_amd import lifting
    rec, vel, tokens, classes = _records_and_velocities()
    meta = {"use_camera": True}
    as_dicts = json.dumps({"meta": meta, "results": lifting.nuscenes_boxes_from_records(rec, tokens, classes, vel=vel)})
    text, n = lifting.nuscenes_results_json(rec, tokens, classes, meta, vel=vel)
    native = lifting.nuscenes_results_json_native(rec, tokens, classes, meta, vel=vel)
    assert n == len(rec) and text == as_dicts and native == text.encode()
    assert '"velocity": [0.0, 0.0]' in text and '"velocity": [-0.0, 0.0]' in text and '"velocity": [3.0, -4.0]' in text
    assert '"velocity": [Infinity, 1.0]' in text and '"velocity": [-Infinity, NaN]' in text and '"velocity": [0, 0]' not in text
    # the per-batch parts of the entry point carry their part's velocities
    parts = []
    for first, count in ((0, 3), (3, 2), (5, 2)):
        sel = (rec[:, 5] >= first) & (rec[:, 5] < first + count)
        parts.append(lifting.nuscenes_results_json_native(rec[sel], tokens, classes, None, part=(first, count), vel=vel[sel]))
    assert lifting.nuscenes_results_json_head(meta) + b", ".join(parts) + b"}}" == native
    with pytest.raises(ValueError):
        lifting.nuscenes_results_json(rec, tokens, classes, meta, vel=vel[:-1])


def test_writers_without_velocities_write_todays_bytes():
    from cm3d_amd import lifting
    rec, vel, tokens, classes = _records_and_velocities()
    meta = {"use_camera": True}
    boxes = lifting.nuscenes_boxes_from_records(rec, tokens, classes)
    assert all(b["velocity"] == [0, 0] and type(b["velocity"][0]) is int for bs in boxes.values() for b in bs)
    text, _ = lifting.nuscenes_results_json(rec, tokens, classes, meta)
    assert text == json.dumps({"meta": meta, "results": boxes}) and text.count('"velocity": [0, 0], "detection_name"') == len(rec)
    assert lifting.nuscenes_results_json_native(rec, tokens, classes, meta) == text.encode()
    assert lifting.nuscenes_results_json_native(rec, tokens, classes, meta, vel=None) == text.encode()
    # the same records with all-zero velocities differ only in the spelling of the zeros
    zeros, _ = lifting.nuscenes_results_json(rec, tokens, classes, meta, vel=np.zeros((len(rec), 2)))
    assert zeros.replace('"velocity": [0.0, 0.0]', '"velocity": [0, 0]') == text


def test_native_tables_expose_next_and_timestamp(tmp_path):
    """reader.Tables.sample_links against the Python tables on the synthetic scene: the native route's frame_next / frame_time equal
    the Python route's."""
    from cm3d_amd import nusc_io, reader, synthetic as syn
    dataroot, _, _ = nusc_io.write_synthetic_dataset(str(tmp_path), syn.config("tiny"), n_scenes=2, frames_per_scene=3, lane_points=200)
    tables = nusc_io.NuscTables("v1.0-synth", dataroot, annotations=False)
    nt = reader.Tables(reader.Reader(2), dataroot, "v1.0-synth")
    names = nt.scene_names()
    tokens, rows = nt.job_tokens(names)
    nxt, ts = nt.sample_links(rows)
    samples = [tables.get("sample", t) for t in tokens]
    assert ts.dtype == np.int64 and ts.tolist() == [s["timestamp"] for s in samples]
    assert V.frame_next_of_rows(rows, nxt).tolist() == V.frame_next_of(tokens, [s["next"] for s in samples]).tolist() == [1, 2, -1, 4, 5, -1]
    assert V.frame_times(ts).tolist() == [0.0, 0.5, 1.0, 0.0, 0.5, 1.0]
    assert V.frame_next_of_rows(rows[[0, 2, 3]], nxt[[0, 2, 3]]).tolist() == [-1, -1, -1]      # followers outside the batch
    with pytest.raises(reader.ReaderError):
        nt.sample_links([len(tables.t["sample"])])
