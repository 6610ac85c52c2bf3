"""The composed CPU pass with the point ownership, for the pass tests of LiftEngine(owner=PointOwner(...)): the two-frame nuScenes and
Waymo batches of tests/box_ground_cases.py (pass_batch), and ground_strip_pass_cases.expected / optin_pass_cases.expected extended by
the ownership -- imported and extended here, not edited:
  1. the oracle's plain pass: raw lists, the cloud, plain medoids and boxes;
  2. pointowner.point_owner_host on the oracle's lists with hb.mask_off and hb.score -> ow_*;
  3. strip: the grid and groundstrip.strip_lists on the exclusive lists -> gs_*;
  4. cluster: cluster.cluster_lists on the lists that are left -> cl_*;
  5. per mask oracle.medoid over the lists that are left -> medoid_pos (a position in them), centroid;
  6. per frame the oracle's stage 2 on those -> lane_idx, lane_dist, box, flags.
Steps 3 to 6 are the imported expectations' own, handed the exclusive lists as the lists of the pass.  Nothing comes from the device."""
import numpy as np

from cm3d_amd import pointowner as po
from tests import box_ground_cases as bgc
from tests import ground_strip_pass_cases as gpc
from tests import optin_pass_cases as oc

OWNER = po.PointOwner()
OW_KEYS = ("ow_off", "ow_status", "ow_lost", "ow_owner", "ow_idx", "ow_xyz")
_EXPECTED = {}


def batch(name):
    return bgc.pass_batch(name)


def plain(orc, name):
    return bgc.pass_plain(orc, name)


def max_pts(hb):
    """The most rows a frame of the batch has: the P the engine hands the stage."""
    return int(max(hb.sweep_row_off[hb.frame_sweep_off[1:]] - hb.sweep_row_off[hb.frame_sweep_off[:-1]]))


def expected(orc, b, base, owner=OWNER, strip=None, cluster=None):
    """Arrays shaped like LiftEngine.download(full=True) of an engine with owner= and these options (plus `ow_tile_off`, `keep` and, as
    the imported expectations add them, `gs_tile_off`, `cl_tile_off`).  base: the oracle's plain pass over the batch."""
    hb = b.hb
    res = po.point_owner_host(base["hit_idx"], base["hit_off"], hb.mask_off, hb.score, max_pts(hb), owner.rule, owner.min_keep)
    keep = res["keep"]
    own = dict(res, ow_idx=base["hit_idx"][keep], ow_xyz=oc.hit_xyz_of(hb, base)[keep])
    owned = dict(base, hit_off=res["ow_off"], hit_idx=own["ow_idx"])          # the pass goes on with the exclusive lists
    if strip is not None:
        out = gpc.expected(orc, b, owned, strip, cluster)
    elif cluster is not None:
        out = oc.expected(orc, b.frames, b.lanes, b.frame_lane, hb, cluster=cluster, base=owned)
    else:
        pts, M, off, idx = base["points"], hb.n_masks, res["ow_off"], own["ow_idx"]
        med, cen = np.full(M, -1, np.int32), np.full((M, 3), np.nan, np.float32)
        for m in range(M):
            o, e = int(off[m]), int(off[m + 1])
            if e > o:
                rows = int(base["pt_off"][int(hb.mask_frame[m])]) + idx[o:e]
                med[m] = orc.medoid(pts, rows)
                cen[m] = pts[rows[med[m]], :3]
        out = dict(owned, medoid_pos=med, centroid=np.where(np.isnan(cen), np.float32(0), cen).astype(np.float32))
        out.update(oc.stage2_records(orc, b.frames, b.lanes, b.frame_lane, hb, cen, med))
    return dict(out, hit_off=base["hit_off"], hit_idx=base["hit_idx"], **own)


def expected_of(orc, name, owner=OWNER, strip=None, cluster=None):
    """expected() of pass_batch(name), once per process (read-only arrays)."""
    key = (name, owner.rule, owner.min_keep, strip is not None, oc._cluster_key(cluster))
    if key not in _EXPECTED:
        _EXPECTED[key] = oc._frozen(expected(orc, batch(name), plain(orc, name), owner, strip, cluster))
    return _EXPECTED[key]


def read_lists(exp):
    """(xyz (n, 4) float32, off) of the lists the stages behind the seam read in an expectation: cl_*, else gs_*, else ow_*."""
    for k in ("cl", "gs", "ow"):
        if k + "_off" in exp:
            xyz = np.asarray(exp[k + "_xyz"], np.float32)
            xyz4 = np.zeros((len(xyz), 4), np.float32)
            xyz4[:, :xyz.shape[1]] = xyz
            return xyz4, exp[k + "_off"]
    raise KeyError("an expectation without exclusive lists")


def contested(exp, hb):
    """(listed points, points in more than one list) of an expectation's raw lists, over the frames of the batch."""
    listed = shared = 0
    for f in range(hb.n_frames):
        lo, hi = int(exp["hit_off"][hb.mask_off[f]]), int(exp["hit_off"][hb.mask_off[f + 1]])
        _, cnt = np.unique(exp["hit_idx"][lo:hi], return_counts=True)
        listed, shared = listed + len(cnt), shared + int((cnt > 1).sum())
    return listed, shared
