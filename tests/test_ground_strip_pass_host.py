"""CPU: what the batches of the stripped pass's GPU tests hold (tests/ground_strip_pass_cases.py: the composed CPU pass on the two-frame
nuScenes and Waymo batches with a ground sheet under the objects).  Each batch contains a list stripped of points, a list with nothing
to strip, a list kept whole and an empty list; the medoid of at least one mask moves; the strip is composed in front of the
clustering; and a mask the vertical stage gives up on because its list holds ground (r > hi) is judged once the ground is gone."""
import numpy as np
import pytest

from cm3d_amd import boxvertical as bv
from cm3d_amd import cluster as clustermod
from tests import ground_strip_pass_cases as pc
from tests import optin_pass_cases as oc


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.mark.parametrize("name", ["nusc", "waymo"])
def test_batches_hold_every_outcome_of_the_strip(orc, name):
    b, base, e = pc.batch(name), pc.plain(orc, name), pc.expected_of(orc, name)
    st, dr = e["gs_status"], e["gs_dropped"]
    n = np.diff(base["hit_off"])
    assert ((st == 0) & (dr > 0)).sum() >= 5 and ((st == 0) & (dr == 0)).sum() >= 2 and (st == 1).sum() >= 2 and (st == 2).sum() >= 1
    assert np.array_equal(st == 2, n == 0) and np.array_equal(np.diff(e["gs_off"]), n - dr) and not dr[st != 0].any()
    assert (np.diff(e["gs_off"])[n > 0] > 0).all()                      # a non-empty list never becomes empty
    assert np.array_equal(e["medoid_pos"] >= 0, base["medoid_pos"] >= 0) and np.array_equal(e["flags"] & 1, base["flags"] & 1)
    moved = (e["centroid"] != base["centroid"]).any(1)
    assert moved.sum() >= 5 and not moved[dr == 0].any()
    # the sheet under the objects gives the grid its estimates, and the stripped points are the low ones
    assert np.isfinite(e["grid_z"]).sum() > 500 and e["grid_z"].shape == (b.hb.n_frames, 4096)
    xyz = oc.hit_xyz_of(b.hb, base)
    for m in np.flatnonzero(dr > 0)[:5]:
        o, g = int(base["hit_off"][m]), int(e["gs_off"][m])
        assert e["gs_xyz"][g:g + int(n[m] - dr[m]), 2].min() >= xyz[o:o + int(n[m]), 2].min()


def test_the_clustering_reads_the_stripped_lists(orc):
    c = clustermod.DepthCluster(1.0, 20)
    e = pc.expected_of(orc, "nusc", cluster=c)
    assert (np.diff(e["cl_off"]) <= np.diff(e["gs_off"])).all() and int(e["cl_off"][-1]) < int(e["gs_off"][-1])
    xyz, off = pc.read_lists(e)
    assert off is e["cl_off"] and len(xyz) == int(e["cl_off"][-1])
    xyz, off = pc.read_lists(pc.expected_of(orc, "nusc"))
    assert len(xyz) == int(off[-1]) and off.tobytes() == pc.expected_of(orc, "nusc")["gs_off"].tobytes()


def test_a_mask_the_vertical_stage_gave_up_on_is_judged_without_its_ground(orc):
    """Without the strip: vert_src 0 with vert_status 0 and r = (top - bottom) / h0 > hi -- "the list holds ground or a wall".  With it
    the same mask is judged."""
    V = bv.BoxVertical()
    b, base, e = pc.batch("nusc"), pc.plain(orc, "nusc"), pc.expected_of(orc, "nusc")
    hx = oc.hit_xyz_of(b.hb, base)
    x4 = np.zeros((len(hx), 4), np.float32)
    x4[:, :hx.shape[1]] = hx
    args = (b.classes.prior_wlh, V.q_bot, V.q_top, V.min_points, V.lo, V.hi)
    v0 = bv.box_vertical_host(x4, base["hit_off"], len(x4), base["box"], base["flags"], *args)
    xs, off = pc.read_lists(e)
    v1 = bv.box_vertical_host(xs, off, len(xs), e["box"], e["flags"], *args)
    h0 = b.classes.prior_wlh[b.hb.class_id, 2]
    with np.errstate(invalid="ignore", divide="ignore"):
        r0 = (v0["vert_z"][:, 1] - v0["vert_z"][:, 0]) / h0
    gave_up = (v0["vert_src"] == 0) & (v0["vert_status"] == 0) & ((base["flags"] & 1) != 0) & (r0 > V.hi)
    assert gave_up.sum() >= 1 and (gave_up & (v1["vert_src"] > 0)).sum() >= 1
