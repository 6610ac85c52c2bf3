"""Frames for the camera records the projection kernel's culling does NOT cover, and for the ones next to its switches
(csrc/project.hip wedge_setup: view wedge, approximate projection, the depth it may accept -- each switched off per camera
when the record is outside what its derivation covers).  tests/test_camera_cases_host.py proves on the CPU that every case
reaches the branch it is meant for and that its crafted rows fall on both sides of every limit; tests/test_gpu_camera_cases.py
runs them on the GPU.  Host only: nothing here touches the device.

The builders generalise tests/magnitude_cases.py's `_craft`: the back-projection goes through the full 3x3 K, the stage
composition is inverted (not transposed: a stage need not be a rotation), and the minimum depth is a parameter."""
import copy

import numpy as np

from cm3d_amd import geometry as geo, rle as rlemod, synthetic as syn
from tests.magnitude_cases import H, N_EACH, N_KINDS, RECT, W, _compose, _rect_rle

N_FRAMES = 3
CAM_K = 45
RECT_KINDS = (4, 5, 6, 7, 9)          # crafted kinds whose limit is an edge of RECT's eroded box (the others: the whole image's)


# ---------------------------------------------------------------------------------------------------------------- records
def _k(rec):
    return rec[CAM_K:CAM_K + 9]


def covered(rec):
    return rec.copy()


def skew(rec):
    r = rec.copy()
    r[CAM_K + 1] = np.float32(0.02) * r[CAM_K]
    return r


def krow3(rec):
    r = rec.copy()
    r[CAM_K + 6] = np.float32(1e-3)
    return r


def k_tiny(rec):
    r = rec.copy()
    r[CAM_K:CAM_K + 9] = _k(r) * np.float32(2.0 ** -110)          # exact: a power of two, nothing goes denormal
    return r


def k_huge(rec):
    r = rec.copy()
    r[CAM_K:CAM_K + 9] = _k(r) * np.float32(2.0 ** 100)
    return r


def shear(rec):
    r = rec.copy()
    S = np.eye(3)
    S[0, 1] = 0.05                                                # camera x += 5 % of camera y
    r[18:27] = (S @ r[18:27].astype(np.float64).reshape(3, 3)).astype(np.float32).reshape(9)
    return r


def near_rot(rec):
    r = rec.copy()
    r[18:27] = (r[18:27].astype(np.float64) * 1.0001).astype(np.float32)
    return r


def stages_3_5(rec):
    """A third stage that is the identity, without translations."""
    r = rec.copy()
    r[30:45] = 0
    r[33:42] = np.eye(3, dtype=np.float32).reshape(9)
    r[54], r[55] = 3, 5
    return r


def stages_3_37(rec):
    """The identity stage with a zero t_post (flag bit 5)."""
    r = stages_3_5(rec)
    r[55] = 37
    return r


def stages_2_15(rec):
    """Split translations: stage 1's t_pre rides as stage 0's t_post (the same addition at the same place in the chain), and the
    two slots that are left hold zeros."""
    r = rec.copy()
    r[12:15] = r[15:18]
    r[15:18] = 0
    r[27:30] = 0
    r[55] = 15
    return r


def stages_1_3(rec):
    """The same rigid map as ONE stage with t_pre and t_post: R = f32(R2 R1), t_pre = t1, t_post = f32(R2 t2).  (Another float32
    chain than the control's, so its lists agree with the control's except next to a limit; the other stages_* classes are
    bit-identical to it.)"""
    t1, R1, _ = geo.cam_stage(rec, 0)
    t2, R2, _ = geo.cam_stage(rec, 1)
    r = rec.copy()
    r[0:45] = 0
    r[0:3] = t1.astype(np.float32)
    r[3:12] = (R2 @ R1).astype(np.float32).reshape(9)
    r[12:15] = (R2 @ t2).astype(np.float32)
    r[54], r[55] = 1, 3
    return r


def stages_3_53(rec):
    """A REAL third stage (not in the issue's table: the classes above re-express the control, so a chain that dropped the third
    stage would still pass them): 3 degrees about the camera's z axis between a t_pre and a t_post of a few centimetres."""
    r = rec.copy()
    r[30:45] = 0
    r[30:33] = np.array([0.03, -0.02, 0.05], np.float32)
    r[33:42] = geo.rot_z(np.deg2rad(3.0)).astype(np.float32).reshape(9)
    r[42:45] = np.array([-0.01, 0.04, 0.02], np.float32)
    r[54], r[55] = 3, 53
    return r


def tele(rec):
    r = rec.copy()
    r[CAM_K] = r[CAM_K + 4] = np.float32(5000.0)
    return r


# id -> (record -> record, ego magnitude of its frames (None: synthetic's default, ~1.7 km), expected (wedge, approximate projection))
CLASSES = {
    "covered": (covered, None, (True, True)),
    "skew": (skew, None, (False, False)),
    "krow3": (krow3, None, (False, False)),
    "k_tiny": (k_tiny, None, (False, False)),
    "k_huge": (k_huge, None, (False, False)),
    "shear": (shear, None, (False, False)),
    "near_rot": (near_rot, None, (True, False)),
    "stages_3_5": (stages_3_5, None, (True, True)),
    "stages_3_37": (stages_3_37, None, (True, True)),
    "stages_2_15": (stages_2_15, None, (True, True)),
    "stages_1_3": (stages_1_3, None, (True, True)),
    "stages_3_53": (stages_3_53, None, (True, True)),
    "tele": (tele, 10000.0, (True, False)),
}
SAME_AS_CONTROL = ("k_tiny", "k_huge", "stages_3_5", "stages_3_37", "stages_2_15")      # bit for bit, on the same points
DIFFERENT_FROM_CONTROL = ("skew", "krow3", "shear", "stages_3_53")
MIXED = ("covered", "skew", "shear", "near_rot", "k_tiny", "covered")
MIXED_NO_MASK_CAM = 3


# ---------------------------------------------------------------------------------------------------------------- the gates
def culling_gates(record, W, H, min_dist):
    """numpy restatement of wedge_setup's decisions for one camera record: float64 composition, float32 where the device code
    rounds to float32.  Returns a dict: plain, dev, omax, zmin (float32), margin_px (0 when the approximate projection is off),
    wedge, apx."""
    f32 = np.float32
    rec = np.asarray(record, np.float32)
    K = rec[CAM_K:CAM_K + 9]
    M, c = _compose(rec)
    o = -(M.T @ c)
    plain = bool(K[1] == 0 and K[3] == 0 and K[6] == 0 and K[7] == 0 and K[8] == 1 and K[0] > 0 and K[4] > 0)
    G = M @ M.T - np.eye(3)
    dev = float(np.abs(G).max())
    omax = f32(np.abs(o).max())
    zmin = f32(f32(f32(min_dist) - f32(0.05)) - f32(f32(1e-4) * omax))
    wedge = plain and dev < 1e-3
    apx, margin = False, 0
    if wedge and zmin > f32(0.1) and dev < 1e-5:
        delta = f32(f32(f32(1e-6) * omax) + f32(1e-4))
        mg = f32(1.0) + np.ceil(f32(f32(f32(f32(2.0) * max(K[0], K[4])) * delta) / zmin))
        if mg < 64.0:
            apx, margin = True, int(mg)
    return dict(plain=plain, dev=dev, omax=omax, zmin=zmin, margin_px=margin, wedge=bool(wedge), apx=apx)


def frame_gates(fr, min_dist):
    """What the frame table holds for `fr` (cm3d_project_culling): bit masks over the cameras, the largest margin, the smallest zmin."""
    g = [culling_gates(r, fr.width, fr.height, min_dist) for r in fr.cams]
    has = 0
    for c in set(int(c) for c in fr.cam_nums if 0 <= c < len(g)):       # (every camera with a mask has the whole-image one: non-empty)
        has |= 1 << c
    return dict(apx_ok=sum(1 << c for c, x in enumerate(g) if x["apx"]), wedge=sum(1 << c for c, x in enumerate(g) if x["wedge"]),
                margin_px=max(x["margin_px"] for x in g), zmin=np.float32(min(x["zmin"] for x in g)), cam_has=has, per_cam=g)


# ---------------------------------------------------------------------------------------------------------------- crafted rows
def craft_rows(fr, rng, W, H, rect, n_each, mag, min_dist, jitter=0.03):
    """tests/magnitude_cases._craft for ANY camera record: sensor-frame rows (n,5) float32 whose exact-arithmetic images sit on
    the culling boundaries of every camera of `fr` -- the same ten kinds in the same order (u, v at the image's accept limits;
    the four edges of `rect`'s eroded box; depth within dz of `min_dist`, anywhere in the image and inside `rect`).
    Pixel (u, v) at depth z is K p = lambda (u, v, 1) with p_z = z, whatever K holds; p_cam = M p + c is solved for p."""
    xf = np.asarray(fr.sweep_xf[0], np.float64)
    R_cs, t_cs, R_ego, t_ego = xf[0:9].reshape(3, 3), xf[9:12], xf[12:21].reshape(3, 3), xf[21:24]
    ex0, ey0, ex1, ey1 = rect[0] + 1, rect[1] + 1, rect[2] - 1, rect[3] - 1          # after the 3x3 erosion
    rows = []
    for c in range(fr.cams.shape[0]):
        M, cv = _compose(fr.cams[c])
        Minv = np.linalg.inv(M)
        Kinv = np.linalg.inv(geo.cam_K(fr.cams[c]))
        jit = lambda n: rng.uniform(-jitter, jitter, n)
        anyu, anyv = lambda n: rng.uniform(2.0, W - 3.0, n), lambda n: rng.uniform(2.0, H - 3.0, n)
        logz = lambda n: np.exp(rng.uniform(np.log(min_dist * 1.005 + 0.01), np.log(90.0), n))
        n = n_each
        dz = 2e-4 + 3e-7 * mag        # the float32 records round the camera's position by up to an ulp of the magnitude
        targets = [
            (1.0 + jit(n), anyv(n), logz(n)), (W - 1.0 + jit(n), anyv(n), logz(n)),
            (anyu(n), 1.0 + jit(n), logz(n)), (anyu(n), H - 1.0 + jit(n), logz(n)),
            (ex0 + jit(n), rng.uniform(ey0, ey1 + 1, n), logz(n)), (ex1 + 1.0 + jit(n), rng.uniform(ey0, ey1 + 1, n), logz(n)),
            (rng.uniform(ex0, ex1 + 1, n), ey0 + jit(n), logz(n)), (rng.uniform(ex0, ex1 + 1, n), ey1 + 1.0 + jit(n), logz(n)),
            (anyu(n), anyv(n), min_dist + rng.uniform(-dz, dz, n)),
            (rng.uniform(ex0, ex1 + 1, n), rng.uniform(ey0, ey1 + 1, n), min_dist + rng.uniform(-dz, dz, n)),
        ]
        for u, v, z in targets:
            q = np.stack([u, v, np.ones_like(u)], 1) @ Kinv.T     # K^-1 (u, v, 1), row form
            pc = q * (z / q[:, 2])[:, None]
            pg = (pc - cv) @ Minv.T
            ps = ((pg - t_ego) @ R_ego - t_cs) @ R_cs            # inverse of sensor -> ego -> global
            rows.append(ps)
    ps = np.concatenate(rows, 0).astype(np.float32)
    k = rng.integers(-4, 5, size=ps.shape).astype(np.int32)      # a few float32 ulps of extra scatter in the sensor frame
    ps = (ps.view(np.int32) + k).view(np.float32)
    out = np.zeros((ps.shape[0], 5), np.float32)
    out[:, :3] = ps
    out[:, 3] = 7.0
    return out


def _scatter(fr, rng, rows):
    """Half of `rows` one by one among sweep 0's ordinary rows, half as one block at its end (magnitude_cases.crafted_frames)."""
    base = fr.sweeps_raw[0]
    order = rng.permutation(rows.shape[0])
    half = rows.shape[0] // 2
    pos = np.sort(rng.choice(base.shape[0], half, replace=False))
    mixed = np.insert(base, pos, rows[order[:half]], axis=0)
    fr.sweeps_raw[0] = np.ascontiguousarray(np.concatenate([mixed, rows[order[half:]]], 0))


def _whole_rle(W, H):
    return {"size": [W, H], "counts": rlemod.counts_to_string(np.array([0, W * H], np.uint32))}


def _add_mask(fr, rl, cam, label="car", score=0.5):
    fr.rles.append(rl); fr.labels.append(label); fr.scores.append(score); fr.cam_nums.append(cam)


def _magnitude(fr):
    return float(np.hypot(*fr.ego_xyz[:2]))


def build_frames(cam_fns, mag=None, min_dist=2.3, seed=0, mask_cams=None, n_frames=N_FRAMES, jitter=0.03):
    """`n_frames` 512x288 frames whose camera c is cam_fns[c] applied to a nuScenes-shaped record; per camera of `mask_cams` (default:
    all) a whole-image mask and RECT behind the synthetic frame's own six masks (those of other cameras are left out);
    N_KINDS x N_EACH crafted rows per camera in sweep 0, half scattered, half in a block.
    Returns (frames, crafted rows per frame).  fr.meta["base_cams"] keeps the unmodified records."""
    n_cams = len(cam_fns)
    cfg = syn.config("tiny", n_points=9000, n_sweeps=2, n_masks=6, n_cams=n_cams, width=W, height=H, ratio=0.32, ego_magnitude=mag,
                     point_order="firing")
    rng = np.random.default_rng(1000 + seed)
    frames, crafted_all = [], []
    for i in range(n_frames):
        fr = syn.make_frame(cfg, 900 + i)
        keep = [k for k, c in enumerate(fr.cam_nums) if mask_cams is None or c in mask_cams]
        fr.rles, fr.labels, fr.scores, fr.cam_nums = ([x[k] for k in keep] for x in (fr.rles, fr.labels, fr.scores, fr.cam_nums))
        fr.meta["base_cams"] = fr.cams.copy()
        fr.cams = np.stack([fn(fr.cams[c]) for c, fn in enumerate(cam_fns)]).astype(np.float32)
        crafted = craft_rows(fr, rng, W, H, RECT, N_EACH, _magnitude(fr), min_dist, jitter)
        _scatter(fr, rng, crafted)
        for c in (range(n_cams) if mask_cams is None else mask_cams):
            _add_mask(fr, _whole_rle(W, H), c, "car", 0.5)
            _add_mask(fr, _rect_rle(*RECT, W, H), c, "human", 0.4)
        frames.append(fr)
        crafted_all.append(crafted)
    return frames, crafted_all


def class_frames(name, min_dist=2.3, n_cams=6, n_frames=N_FRAMES):
    """Uniform frames: class `name` on every camera."""
    fn, mag, _ = CLASSES[name]
    return build_frames([fn] * n_cams, mag, min_dist, seed=sorted(CLASSES).index(name) + 10 * n_cams, n_frames=n_frames)


def straddling_min_dists(n_frames=N_FRAMES):
    """Two minimum depths around the one at which a covered camera's zmin crosses 0.1 at the frames' magnitude: with the lower one
    EVERY camera of every frame has the approximate projection off (zmin <= 0.1), with the higher one every camera has it on."""
    frames, _ = class_frames("covered", n_frames=n_frames)
    omax = [float(culling_gates(r, W, H, 2.3)["omax"]) for fr in frames for r in fr.cams]
    return round(0.15 + 1e-4 * min(omax) - 0.01, 3), round(0.15 + 1e-4 * max(omax) + 0.01, 3)


def min_dist_values():
    lo, hi = straddling_min_dists()
    return [lo, hi, 1.0, 5.0]


def mixed_frames(variant="plain", n_frames=N_FRAMES):
    """Cameras 0..5 = MIXED; camera 3 has no mask.  variant:
      "plain"    nothing else
      "bad_cam"  one more mask per frame whose camera number is n_cams (out of range: no points, status bit 2)
      "many"     more than 64 masks (three hit-word planes): 38 more small rectangles on camera 1 (skew; 40 entries) and 31 more
                 on camera 0 (covered; 33 entries, so the pre-test of more than 32 entries is skipped)
      "garbage"  rows no camera sees scattered through sweep 0: 4 each of all-NaN, x = +inf, z = -inf, 1e6 m along the optical
                 axis of cameras 0, 5, 1, 4, and coordinates of 1e-40
    Returns (frames, crafted rows per frame, garbage rows per frame or None)."""
    fns = [CLASSES[n][0] for n in MIXED]
    frames, crafted = build_frames(fns, None, 2.3, seed=77, mask_cams=[c for c in range(6) if c != MIXED_NO_MASK_CAM], n_frames=n_frames)
    rng = np.random.default_rng(4242)
    garbage = None
    for fr in frames:
        if variant == "bad_cam":
            _add_mask(fr, _rect_rle(40, 30, 470, 250, W, H), fr.cams.shape[0], "car", 0.6)
        elif variant == "many":
            for k in range(38):
                x0, y0 = 20 + 60 * (k % 8), 20 + 50 * (k // 8)
                _add_mask(fr, _rect_rle(x0, y0, x0 + 45, y0 + 38, W, H), 1, "car", 0.3 + 0.01 * k)
            for k in range(31):
                x0, y0 = 8 + 62 * (k % 8), 30 + 60 * (k // 8)
                _add_mask(fr, _rect_rle(x0, y0, x0 + 50, y0 + 44, W, H), 0, "human", 0.3 + 0.01 * k)
        elif variant == "garbage":
            garbage = garbage or []
            g = garbage_rows(fr)
            _scatter(fr, rng, g)
            garbage.append(g)
        elif variant != "plain":
            raise ValueError(variant)
    return frames, crafted, garbage


GARBAGE_KINDS = ("nan", "x_inf", "z_minf", "far", "denormal")
GARBAGE_FAR_CAMS = (0, 5, 1, 4)


def garbage_rows(fr):
    """(20, 5) float32 sensor-frame rows, 4 per kind of GARBAGE_KINDS, in that order.  The far ones lie 1e6 m along the optical axis
    (through the image centre) of the cameras GARBAGE_FAR_CAMS; the intensity column numbers them, 1000 + row (ordinary rows: < 256)."""
    xf = np.asarray(fr.sweep_xf[0], np.float64)
    R_cs, t_cs, R_ego, t_ego = xf[0:9].reshape(3, 3), xf[9:12], xf[12:21].reshape(3, 3), xf[21:24]
    rows = np.zeros((20, 5), np.float32)
    rows[0:4, :3] = np.nan
    rows[4:8, :3] = [[np.inf, 3.0, -1.0], [np.inf, -20.0, 0.5], [np.inf, 0.0, 0.0], [np.inf, 55.0, 2.0]]
    rows[8:12, :3] = [[4.0, 3.0, -np.inf], [-30.0, 1.0, -np.inf], [2.0, -3.0, -np.inf], [12.0, -40.0, -np.inf]]
    for j, c in enumerate(GARBAGE_FAR_CAMS):
        M, cv = _compose(fr.cams[c])
        q = np.linalg.inv(geo.cam_K(fr.cams[c])) @ np.array([0.5 * fr.width, 0.5 * fr.height, 1.0])
        pg = np.linalg.inv(M) @ (q * (1e6 / q[2]) - cv)
        rows[12 + j, :3] = (((pg - t_ego) @ R_ego - t_cs) @ R_cs).astype(np.float32)
    rows[16:20, :3] = np.float32(1e-40) * np.array([[1, 1, 1], [-1, 2, 3], [5, -7, 0], [0, 0, 9]], np.float32)
    rows[:, 3] = 1000.0 + np.arange(20)
    return rows


def oracle_view(frames):
    """The frames as the oracle can take them: a mask of an out-of-range camera (which gets no points) becomes an empty mask on camera
    0.  Returns (frames, batch numbers of the replaced masks)."""
    out, bad, m = [], [], 0
    for fr in frames:
        f2 = copy.copy(fr)
        f2.rles, f2.cam_nums = list(fr.rles), list(fr.cam_nums)
        for k, c in enumerate(fr.cam_nums):
            if not 0 <= c < fr.cams.shape[0]:
                f2.rles[k] = {"size": [fr.width, fr.height], "counts": rlemod.counts_to_string(np.array([fr.width * fr.height], np.uint32))}
                f2.cam_nums[k] = 0
                bad.append(m + k)
        m += len(fr.rles)
        out.append(f2)
    return out, bad


# ---------------------------------------------------------------------------------------------------------------- oracle-side accounting
def eroded_masks(orc):
    """(whole image, RECT) after the 3x3 erosion, (H, W) uint8."""
    rect = np.zeros((H, W), np.uint8)
    rect[RECT[1]:RECT[3] + 1, RECT[0]:RECT[2] + 1] = 1
    return orc.erode3x3(np.ones((H, W), np.uint8)), orc.erode3x3(rect)


def crafted_sides(orc, fr, rows, min_dist):
    """(n_cams, N_KINDS) int: how many of the N_EACH crafted rows of (camera, kind) the oracle puts INSIDE that kind's mask
    (RECT for RECT_KINDS, else the whole image) of that camera."""
    x = fr.sweep_xf[0]
    P = orc.sweep_prep(rows, x[0:9], x[9:12], x[12:21], x[21:24], np.float32(0.0))
    n_cams = fr.cams.shape[0]
    assert P.shape[0] == rows.shape[0] == n_cams * N_KINDS * N_EACH
    full, rect = eroded_masks(orc)
    out = np.zeros((n_cams, N_KINDS), np.int64)
    for c in range(n_cams):
        in_img = np.zeros(P.shape[0], bool); in_img[orc.points_in_mask(P, fr.cams[c], full, min_dist)] = True
        in_rect = np.zeros(P.shape[0], bool); in_rect[orc.points_in_mask(P, fr.cams[c], rect, min_dist)] = True
        for kind in range(N_KINDS):
            sel = slice((c * N_KINDS + kind) * N_EACH, (c * N_KINDS + kind + 1) * N_EACH)
            out[c, kind] = int((in_rect if kind in RECT_KINDS else in_img)[sel].sum())
    return out


def frame_cloud(orc, fr, min_dist):
    """The frame's aggregated cloud as the reference builds it (ego box of half width f32(sqrt(min_dist)))."""
    halfw = np.float32(np.sqrt(min_dist))
    return np.concatenate([orc.sweep_prep(r, x[0:9], x[9:12], x[12:21], x[21:24], halfw) for r, x in zip(fr.sweeps_raw, fr.sweep_xf)], 0)
