"""GPU: the opt-in passes of a LiftEngine -- clustered, filtered, both, and the rotated-box NMS behind each -- against the composed CPU
expectation of tests/optin_pass_cases.py, on batches whose lists leave one medoid tile, reach the two-pass medoid route and the
clustering's long route, and whose frames take the rotated NMS to an LDS bound between its two tested ones
(tests/test_optin_pass_cases_host.py asserts that the batches do).  Every comparison is exact; the box columns get
tests/test_gpu_parity.py's tolerance, through its own function."""
import numpy as np
import pytest

from cm3d_amd import cluster as clustermod
from cm3d_amd import nms as nmsmod
from tests import optin_pass_cases as oc
from tests.test_gpu_parity import _compare_box, _compare_raw

pytestmark = pytest.mark.gpu

POISON = ("cl_off", "cl_tile_off", "cl_idx", "cl_status", "medoid_pos", "flags", "lane_idx")


def _sync_download(eng):
    import torch
    torch.cuda.synchronize()
    out = eng.download(full=True)
    if eng.cluster is not None:
        out["cl_tile_off"] = eng.b.cl_tile_off.cpu().numpy()
    return out


def _run(eng, hb=None):
    if hb is not None:
        eng.upload(hb)
    eng.run(masks="rle")
    return _sync_download(eng)


def _poison(eng):
    """Whatever the next pass does not rewrite would show."""
    for name in POISON:
        if hasattr(eng.b, name):
            getattr(eng.b, name).fill_(-3)
    if eng.cluster is not None:
        eng.b.cl_xyz.fill_(0.0)
    eng.b.centroid.fill_(-3.0)
    eng.b.box.fill_(-3.0)


def _same_bytes(a, b):
    assert set(a) == set(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k


def _check_pass(hb, got, exp):
    """One downloaded pass against the composed expectation: the raw lists (test_gpu_parity's part), the clustered lists to the bit,
    the medoid of the (clustered) lists, stage 2, the filter's outputs, flags; the box columns within test_gpu_parity's tolerance."""
    _compare_raw(hb, got, exp)
    if "cl_off" in exp:
        for key in ("cl_off", "cl_tile_off", "cl_status", "cl_idx"):
            assert got[key].dtype == np.int32 and np.array_equal(got[key], exp[key]), key
        assert got["cl_xyz"].shape == exp["cl_xyz"].shape and np.array_equal(got["cl_xyz"].view(np.uint32), exp["cl_xyz"].view(np.uint32))
    else:
        assert "cl_off" not in got
    assert np.array_equal(got["medoid_pos"], exp["medoid_pos"])
    assert np.array_equal(got["centroid"].view(np.uint32), exp["centroid"].view(np.uint32))
    assert np.array_equal(got["lane_idx"], exp["lane_idx"])
    valid = exp["medoid_pos"] >= 0
    assert np.array_equal(got["lane_dist"][valid], exp["lane_dist"][valid])
    if "medoid_pos_kept" in exp:
        assert np.array_equal(got["medoid_pos_kept"], exp["medoid_pos_kept"])
        assert got["on_road"].dtype == np.uint8 and np.array_equal(got["on_road"], exp["on_road"])
    else:
        assert "medoid_pos_kept" not in got
    assert np.array_equal(got["flags"], exp["flags"])
    _compare_box(got, exp)


# ------------------------------------------------------------------------------------------------ the clustered pass
@pytest.mark.parametrize("name,pick", [("mid", "largest"), ("mid", "nearest"), ("deep", "largest"), ("many", "largest")])
def test_clustered_pass_equals_the_composed_oracle(oracle, name, pick):
    from cm3d_amd import lifting
    b = oc.batch(name)
    c = clustermod.DepthCluster(b.cluster.eps, b.cluster.min_points, pick)
    exp = oc.expected_of(oracle, name, cluster=c)
    eng = lifting.LiftEngine("cuda:0", cluster=c)
    got = _run(eng, b.hb)
    _check_pass(b.hb, got, exp)
    _poison(eng)
    _same_bytes(_run(eng), got)


def test_the_hint_follows_the_clustered_lists(oracle):
    """One engine, eps 1.0: `mid` (raw lists above 448 points, no clustered list above it), `deep` (clustered lists of thousands), `mid`
    again, three passes each -- the first on the hint of the batch before.  Every pass is the expectation's, and the feedback word says
    what the clustered lists are, not the raw ones.  Then `deep` once more through a captured graph."""
    from cm3d_amd import lifting
    c = clustermod.DepthCluster(1.0, 20)
    eng = lifting.LiftEngine("cuda:0", cluster=c)
    seen = []
    for name in ("mid", "deep", "mid"):
        b = oc.batch(name)
        exp = oc.expected_of(oracle, name, cluster=c)
        long_cl = bool(np.diff(exp["cl_off"]).max() > oc.MD_BATCH_LONG)
        assert np.diff(exp["hit_off"]).max() > oc.MD_BATCH_LONG and long_cl == (name == "deep")
        eng.upload(b.hb)
        for _ in range(3):
            got = _run(eng)
            seen.append(int(eng._md_fb_np[0]))
            _check_pass(b.hb, got, exp)
            assert seen[-1] == int(long_cl), (name, seen)
    assert seen == [0, 0, 0, 1, 1, 1, 0, 0, 0]
    b = oc.batch("deep")
    exp = oc.expected_of(oracle, "deep", cluster=c)
    first = _run(eng, b.hb)                                   # (on the hint `mid` left: the one-pass route over lists of thousands)
    _check_pass(b.hb, first, exp)
    g = eng.capture_graph(masks="rle")
    _poison(eng)
    g.replay()
    rep = _sync_download(eng)
    _check_pass(b.hb, rep, exp)
    _same_bytes(rep, first)


# ------------------------------------------------------------------------------------------------ filters behind the clustering
@pytest.mark.parametrize("name", ["mid", "many"])
def test_filters_and_clustering_together_equal_the_composed_oracle(oracle, name):
    from cm3d_amd import lifting
    b = oc.batch(name)
    only = oc.expected_of(oracle, name, cluster=b.cluster)
    f = oc.lane_filters(only)
    exp = oc.expected_of(oracle, name, cluster=b.cluster, filters=f)
    eng = lifting.LiftEngine("cuda:0", filters=f, cluster=b.cluster)
    got = _run(eng, b.hb)
    _check_pass(b.hb, got, exp)
    for key in oc.CLUSTER_KEYS + ("medoid_pos",):            # (the filter changes none of them: the expectation's arrays are the unfiltered ones)
        assert exp[key] is only[key]
    dropped = (got["medoid_pos"] >= 0) & (got["medoid_pos_kept"] < 0)
    assert dropped.sum() >= 3 and (got["medoid_pos_kept"] >= 0).sum() >= 3
    _poison(eng)
    _same_bytes(_run(eng), got)


# ------------------------------------------------------------------------------------------------ the rotated NMS behind each pass
KINDS = {"plain": (False, False), "filters": (False, True), "cluster": (True, False), "both": (True, True)}


def _engine_kw(oracle, name, kind):
    """(LiftEngine's arguments, the composed expectation) of one kind of pass over the batch."""
    b = oc.batch(name)
    clustered, filtered = KINDS[kind]
    c = b.cluster if clustered else None
    exp = oc.expected_of(oracle, name, cluster=c)
    kw = {}
    if clustered:
        kw["cluster"] = c
    if filtered:
        kw["filters"] = oc.lane_filters(exp)
        exp = oc.expected_of(oracle, name, cluster=c, filters=kw["filters"])
    return kw, exp


def _check_nms(hb, both, base, r):
    """both: the pass with the rotated NMS, base: the same pass without.  Everything but bit 1 of flags and column 9 of box is base's
    bytes; the decision is the host statement's on the device's own rows (they equal the oracle's only within 1e-5: overlaps taken from
    the oracle's rows could straddle a threshold; the kernel's exactness is tests/test_gpu_rotated_nms.py's business).  Returns
    (the boxes that took part, keep)."""
    assert set(both) == set(base)
    for key in base:
        if key not in ("box", "flags"):
            assert both[key].dtype == base[key].dtype and both[key].tobytes() == base[key].tobytes(), key
    assert both["box"][:, :9].tobytes() == base["box"][:, :9].tobytes() and np.array_equal(both["flags"] & 1, base["flags"] & 1)
    assert np.array_equal(both["box"][:, 9], both["flags"].astype(np.float64)) and set(np.unique(both["flags"]).tolist()) <= {0, 1, 3}
    keep = oc.rotated_keep(both["box"], both["flags"], hb, r)
    assert np.array_equal(both["flags"] >> 1, keep)
    return (both["flags"] & 1) == 1, keep


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("name", ["many", "mid"])
def test_rotated_nms_behind_every_kind_of_pass(oracle, name, kind):
    from cm3d_amd import lifting
    b = oc.batch(name)
    kw, exp = _engine_kw(oracle, name, kind)
    r = nmsmod.RotatedNms(class_agnostic=True)
    base = _run(lifting.LiftEngine("cuda:0", **kw), b.hb)
    _check_pass(b.hb, base, exp)
    eng = lifting.LiftEngine("cuda:0", nms=r, **kw)
    both = _run(eng, b.hb)
    took, keep = _check_nms(b.hb, both, base, r)
    if name == "many":
        # every frame has more than 64 masks and the launch's bound is 160: 256 threads, records in LDS in a layout of 160 slots
        assert eng.b.planes == 5 and np.diff(b.hb.mask_off).min() > 64
        gone = [int((took & (keep == 0))[int(b.hb.mask_off[f]):int(b.hb.mask_off[f + 1])].sum()) for f in range(b.hb.n_frames)]
        if "filters" in kw:                                  # (the median threshold leaves frame 0 ten boxes: fewer than ten can go there)
            assert sum(gone) >= 10, gone
        else:
            assert min(gone) >= 10, gone
        assert not np.array_equal(both["flags"], base["flags"])
    else:
        assert eng.b.planes == 1
    _poison(eng)
    _same_bytes(_run(eng), both)


def test_rotated_nms_cover_with_per_class_thresholds_at_the_lds_bound(oracle):
    from cm3d_amd import lifting
    b = oc.batch("many")
    kw, exp = _engine_kw(oracle, "many", "cluster")
    r = nmsmod.RotatedNms(measure="cover", thr={"car": 0.3, "pedestrian": 0.6}, class_agnostic=True)
    base = _run(lifting.LiftEngine("cuda:0", **kw), b.hb)
    _check_pass(b.hb, base, exp)
    eng = lifting.LiftEngine("cuda:0", nms=r, **kw)
    took, keep = _check_nms(b.hb, _run(eng, b.hb), base, r)
    iou = oc.rotated_keep(base["box"], base["flags"], b.hb, nmsmod.RotatedNms(class_agnostic=True))
    assert eng.b.planes == 5 and (took & (keep == 0)).sum() >= 20 and not np.array_equal(keep, iou)


# ------------------------------------------------------------------------------------------------ the OBB fit on the clustered lists
def test_obb_on_clustered_lists_equals_the_canonical_restatement(oracle):
    """LiftEngine(obb=True, cluster=...) on `mid`: cm3d_obb sees the clustered lists.  Status of every list, and the yaw to 1e-9 of the
    lists tests/test_gpu_obb.py's eigenvalue-gap rule does not leave out (tests/test_optin_pass_cases_host.py: at least 20 of them)."""
    from cm3d_amd import kitti as kt, lifting
    from tests.test_gpu_obb import EIG_GAP_MIN, _ang
    b = oc.batch("mid")
    exp = oc.expected_of(oracle, "mid", cluster=b.cluster)
    yaw, st, pinned = oc.obb_expected(exp, EIG_GAP_MIN)
    got = _run(lifting.LiftEngine("cuda:0", obb=True, cluster=b.cluster), b.hb)
    _check_pass(b.hb, got, exp)
    assert np.array_equal(got["obb_status"], st)
    assert np.isnan(got["obb_yaw"][st == kt.OBB_SKIPPED]).all() and np.isfinite(got["obb_yaw"][st == kt.OBB_FITTED]).all()
    err = _ang(got["obb_yaw"][pinned], yaw[pinned])
    print(f"obb: {int(pinned.sum())} lists compared, largest yaw difference {err.max():.3g}")
    assert pinned.sum() >= 20 and err.max() <= 1e-9
    # ... and they are not the raw lists' yaws
    raw = _run(lifting.LiftEngine("cuda:0", obb=True), b.hb)
    lost = np.diff(exp["cl_off"]) < np.diff(exp["hit_off"])
    assert (_ang(raw["obb_yaw"][pinned & lost], yaw[pinned & lost]) > 1e-6).sum() >= 5
