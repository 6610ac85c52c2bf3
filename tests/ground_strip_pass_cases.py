"""The composed CPU pass with the ground strip, for the pass tests of LiftEngine(strip=GroundStrip(...)): the two-frame nuScenes and
Waymo batches of tests/box_ground_cases.py (pass_batch: a tilted ground sheet of rings in every frame, under the objects), and
optin_pass_cases.expected extended by the strip -- imported and extended here, not edited:
  1. the oracle's plain pass: raw lists, the cloud (its sweep preparation), plain medoids and boxes;
  2. groundstrip.ground_grid_host on that cloud with hb.ego_xyz as the origins -> grid_z, grid_n;
  3. groundstrip.strip_lists on the oracle's lists -> gs_*;
  4. cluster: cluster.cluster_lists on the stripped lists -> cl_*;
  5. per mask oracle.medoid over the lists that are left -> medoid_pos (a position in them), centroid;
  6. per frame the oracle's stage 2 on those -> lane_idx, lane_dist, box, flags; filters as optin_pass_cases composes them.
Nothing in it comes from the device."""
import numpy as np

from cm3d_amd import cluster as clustermod
from cm3d_amd import groundstrip as gs
from tests import box_ground_cases as bgc
from tests import optin_pass_cases as oc

STRIP = gs.GroundStrip()
_EXPECTED = {}


def batch(name):
    return bgc.pass_batch(name)


def plain(orc, name):
    return bgc.pass_plain(orc, name)


def expected(orc, b, base, strip=STRIP, cluster=None, filters=None, tables=None):
    """Arrays shaped like LiftEngine.download(full=True) of an engine with strip= and these options (plus `gs_tile_off` and, with a
    cluster, `cl_tile_off`, which the engine keeps in eng.b).  base: the oracle's plain pass over the batch."""
    hb = b.hb
    hit_xyz = oc.hit_xyz_of(hb, base)
    grid_z, grid_n = gs.ground_grid_host(base["points"], base["pt_off"], hb.ego_xyz, strip.cell, strip.down, strip.up, strip.quantile, strip.min_points)
    gs_off, gs_tile_off, keep, status, dropped = gs.strip_lists(base["hit_off"], hit_xyz, hb.mask_frame, hb.ego_xyz, grid_z, strip.cell, strip.margin,
                                                                strip.min_keep)
    out = dict(base, grid_z=grid_z, grid_n=grid_n, gs_off=gs_off, gs_tile_off=gs_tile_off, gs_status=status, gs_dropped=dropped,
               gs_idx=base["hit_idx"][keep], gs_xyz=hit_xyz[keep])
    off, idx = gs_off, out["gs_idx"]
    if cluster is not None:
        cl_off, cl_tile_off, ckeep, cstatus = clustermod.cluster_lists(gs_off, out["gs_xyz"], hb.mask_frame, hb.ego_xyz, cluster.eps, cluster.min_points,
                                                                       cluster.pick)
        out.update(cl_off=cl_off, cl_tile_off=cl_tile_off, cl_status=cstatus, cl_idx=idx[ckeep], cl_xyz=out["gs_xyz"][ckeep])
        off, idx = cl_off, out["cl_idx"]
    pts, M = base["points"], hb.n_masks
    med, cen = np.full(M, -1, np.int32), np.full((M, 3), np.nan, np.float32)
    for m in range(M):
        o, e = int(off[m]), int(off[m + 1])
        if e > o:
            rows = int(base["pt_off"][int(hb.mask_frame[m])]) + idx[o:e]
            med[m] = orc.medoid(pts, rows)
            cen[m] = pts[rows[med[m]], :3]
    out.update(medoid_pos=med, centroid=np.where(np.isnan(cen), np.float32(0), cen).astype(np.float32))
    out.update(oc.stage2_records(orc, b.frames, b.lanes, b.frame_lane, hb, cen, med))
    if filters is not None:
        out = oc._filtered(orc, b.frames, b.lanes, b.frame_lane, hb, out, filters, tables)
    return out


def expected_of(orc, name, cluster=None):
    """expected() of pass_batch(name) at the default strip, once per process (read-only arrays)."""
    key = (name, oc._cluster_key(cluster))
    if key not in _EXPECTED:
        _EXPECTED[key] = oc._frozen(expected(orc, batch(name), plain(orc, name), cluster=cluster))
    return _EXPECTED[key]


def read_lists(exp):
    """(xyz (n, 4) float32, off) of the lists the stages behind the seam read in an expectation: cl_*, else gs_*, else the raw ones."""
    if "cl_off" in exp:
        off, xyz = exp["cl_off"], exp["cl_xyz"]
    elif "gs_off" in exp:
        off, xyz = exp["gs_off"], exp["gs_xyz"]
    else:
        raise KeyError("an expectation without stripped lists")
    xyz = np.asarray(xyz, np.float32)
    xyz4 = np.zeros((len(xyz), 4), np.float32)
    xyz4[:, :xyz.shape[1]] = xyz
    return xyz4, off
