"""Host side of the opt-in box size stage (include/cm3d_hip.h: cm3d_box_size; the call behind cm3d_box_tracks).

Every box the pass writes has the size of its class prior.  The yaw fit (bevfit.YawFit) leaves the extents of a vehicle's points at
the fitted heading, the placement (boxplace.BoxPlace) hangs the prior on that rectangle, and the track stage (tracks.Tracks) says which
boxes are one object.  Here the extent / prior ratios of a track are pooled -- an upper order statistic, because one frame's extent is a
lower bound with outliers --, the pooled size is hung on the rectangle by the placement's rule, and the velocity is taken again on the
new centres.  This module is the rule's statement to the bit (box_size_host), the switches of the stage (BoxSize) and the flags of the
entry points.  The device result is held against it, never the other way round.

The four defaults (q = 0.75, min_obs = 2, lo = 0.6, hi = 1.5) are untuned, and what the stage does to label quality has not been
measured: it cannot be on synthetic scenes.
"""
from dataclasses import dataclass

import numpy as np

from ._lib import BOX_STRIDE

STATUS_LINK, STATUS_CUT = 1, 2            # a link, head or membership that is none; a walk cut at n_frames steps
SRC_LENGTH, SRC_WIDTH = 1, 2              # size_src bits: the dimension was pooled
MODES = ("prior", "track")                # --size
DEFAULT_Q, DEFAULT_MIN_OBS, DEFAULT_LO, DEFAULT_HI = 0.75, 2, 0.6, 1.5      # untuned


def _check(q, min_obs, lo, hi):
    if not (0.0 <= q <= 1.0):
        raise ValueError("q: in [0, 1]")
    if int(min_obs) < 1:
        raise ValueError("min_obs >= 1")
    if not (0.0 < lo <= hi and np.isfinite(hi)):
        raise ValueError("0 < lo <= hi, both finite")


@dataclass
class BoxSize:
    """The opt-in size stage (behind yaw=YawFit(...), place=BoxPlace(...), velocity=Velocity(...) and the track stage): a vehicle box
    whose yaw was fitted takes length and width from its track's pooled extents.  q: the quantile (order statistic, no interpolation)
    of a track's extent / prior ratios; min_obs: fewer observations of a dimension leave it at the prior; lo, hi: a ratio outside
    [lo, hi] is no observation (a face that was not seen, or background in the list).  All four untuned."""
    q: float = DEFAULT_Q
    min_obs: int = DEFAULT_MIN_OBS
    lo: float = DEFAULT_LO
    hi: float = DEFAULT_HI

    def __post_init__(self):
        self.q, self.min_obs, self.lo, self.hi = float(self.q), int(self.min_obs), float(self.lo), float(self.hi)
        _check(self.q, self.min_obs, self.lo, self.hi)

    @property
    def active(self):
        return True


def add_arguments(ap):
    """The flags of the nuScenes entry points; --size prior (the default) is the path without the stage."""
    ap.add_argument("--size", choices=MODES, default="prior",
                    help="prior: every box has its class's size; track (with --yaw fit --place fit --velocity track): length and width "
                         "from the fitted extents pooled over the box's track.  Untuned, quality not measured")
    ap.add_argument("--size-quantile", type=float, default=None, metavar="Q",
                    help=f"with --size track: the order statistic of a track's extent / prior ratios (default {DEFAULT_Q}; untuned)")
    ap.add_argument("--size-min-obs", type=int, default=None, metavar="N",
                    help=f"with --size track: a dimension observed fewer than N times in a track stays the prior's (default {DEFAULT_MIN_OBS}; untuned)")
    ap.add_argument("--size-ratio", default=None, metavar="LO,HI",
                    help=f"with --size track: an extent outside [LO, HI] times the prior is no observation (default {DEFAULT_LO},{DEFAULT_HI}; untuned)")


def from_args(args, ap=None):
    """BoxSize from an entry point's flags; None for --size prior.  --size track without --yaw fit --place fit --velocity track, or a
    --size-* flag without --size track, is an error of the command line (ap.error when the parser is given, else ValueError)."""
    try:
        given = [flag for flag, v in (("--size-quantile", args.size_quantile), ("--size-min-obs", args.size_min_obs),
                                      ("--size-ratio", args.size_ratio)) if v is not None]
        if args.size != "track":
            if given:
                raise ValueError(f"{given[0]} needs --size track")
            return None
        for flag, attr, want in (("--yaw fit", "yaw", "fit"), ("--place fit", "place", "fit"), ("--velocity track", "velocity", "track")):
            if getattr(args, attr, None) != want:
                raise ValueError(f"--size track needs {flag}")
        lo, hi = DEFAULT_LO, DEFAULT_HI
        if args.size_ratio is not None:
            parts = args.size_ratio.split(",")
            if len(parts) != 2:
                raise ValueError(f"--size-ratio: LO,HI expected, got {args.size_ratio!r}")
            lo, hi = float(parts[0]), float(parts[1])
        return BoxSize(DEFAULT_Q if args.size_quantile is None else args.size_quantile,
                       DEFAULT_MIN_OBS if args.size_min_obs is None else args.size_min_obs, lo, hi)
    except ValueError as e:
        if ap is None:
            raise
        ap.error(str(e))


def box_size_host(box, flags, mask_frame, fit_rect, place_src, prior_wlh, ego_xyz, next_match, prev_match, track_id, track_pos, track_len,
                  frame_time, thin=0.5, max_dt=1.5, smooth_window=0, q=DEFAULT_Q, min_obs=DEFAULT_MIN_OBS, lo=DEFAULT_LO, hi=DEFAULT_HI):
    """What cm3d_box_size computes (include/cm3d_hip.h states the rule), to the bit.  ego_xyz (F, 3) on nuScenes, None on Waymo.
    Returns a dict: the new box (a copy; flags comes back as it went in), size_wlh (M, 3), size_src (M,) int32, size_ratio (M, 2),
    size_obs (M, 2) int32, size_placed (M, 2), size_vel (M, 2), status.  numpy rounds every float64 operation on its own: the
    expressions below are the rule's, bracket for bracket."""
    _check(q, min_obs, lo, hi)
    if not (np.isfinite(thin) and thin >= 0.0) or not max_dt > 0.0 or int(smooth_window) < 0:
        raise ValueError("thin finite and >= 0, max_dt > 0, smooth_window >= 0")
    box = np.array(box, np.float64).reshape(-1, BOX_STRIDE)
    M = box.shape[0]
    flags = np.array(flags, np.int32).reshape(M)
    frame = np.asarray(mask_frame, np.int64).reshape(M)
    rect = np.asarray(fit_rect, np.float64).reshape(M, 6)
    psrc = np.asarray(place_src, np.int64).reshape(M)
    prior = np.asarray(prior_wlh, np.float64).reshape(-1, 3)
    nm, pm = np.asarray(next_match, np.int64).reshape(M), np.asarray(prev_match, np.int64).reshape(M)
    tid, pos, ln = (np.asarray(a, np.int64).reshape(M) for a in (track_id, track_pos, track_len))
    time = np.asarray(frame_time, np.float64).reshape(-1)
    F, W = time.size, int(smooth_window)
    if F <= 0 or prior.shape[0] <= 0:
        raise ValueError("n_frames > 0, n_classes > 0")
    q, lo, hi, thin, min_obs = np.float64(q), np.float64(lo), np.float64(hi), np.float64(thin), int(min_obs)
    ego = None if ego_xyz is None else np.asarray(ego_xyz, np.float64).reshape(-1, 3)

    with np.errstate(invalid="ignore"):
        b8 = box[:, 8]
        cls = np.where((b8 >= 0.0) & (b8 < float(prior.shape[0])), b8, 0.0).astype(np.int64)
    wid0, len0 = prior[cls, 0], prior[cls, 1]
    member = (ln > 0) & (tid >= 0) & (tid < M) & (pos >= 0) & (pos < ln) & (frame >= 0) & (frame < F)
    t = np.where(member, time[np.where(member, frame, 0)], 0.0)
    status = 0

    def links(a, step):
        nonlocal status
        out = np.full(M, -1, np.int64)
        for i in np.flatnonzero(member):
            j = int(a[i])
            if 0 <= j < M and member[j] and tid[j] == tid[i] and pos[j] == pos[i] + step:
                out[i] = j
            elif j != -1:
                status |= STATUS_LINK
        return out
    vnext, vprev = links(nm, 1), links(pm, -1)

    # observations: NaN stands for none
    obs = np.full((M, 2), np.nan)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        rl, rw = rect[:, 2] / len0, rect[:, 3] / wid0
        seen = member & (psrc != 0)
        obs[:, 0] = np.where(seen & (len0 > 0.0) & (lo <= rl) & (rl <= hi), rl, np.nan)
        obs[:, 1] = np.where(seen & (wid0 > 0.0) & (lo <= rw) & (rw <= hi), rw, np.nan)

    # tracks: the walk from every head that members name
    size_ratio, size_obs = np.zeros((M, 2), np.float64), np.zeros((M, 2), np.int32)
    pooled = np.zeros((M, 2), bool)
    on_track = np.zeros(M, bool)
    heads = np.unique(tid[member])
    good = {int(h) for h in heads if member[h] and tid[h] == h and pos[h] == 0}
    walks = {}
    for h in good:
        mem, m = [], h
        while m >= 0 and len(mem) < F:
            mem.append(m)
            m = int(vnext[m])
        walks[h] = mem
        ratio, n_of, is_pooled = [np.float64(1.0)] * 2, [0, 0], [False, False]
        for d in (0, 1):
            vals = [(obs[m_, d], k_) for k_, m_ in enumerate(mem) if not np.isnan(obs[m_, d])]
            n_of[d] = len(vals)
            if n_of[d] >= min_obs:
                k = int(q * np.float64(n_of[d] - 1))
                ratio[d], is_pooled[d] = sorted(vals)[k][0], True
        on_track[mem] = True
        size_ratio[mem], size_obs[mem], pooled[mem] = ratio, n_of, is_pooled
    for i in np.flatnonzero(member):
        h = int(tid[i])
        if h in good and len(walks[h]) == F and vnext[walks[h][-1]] >= 0:
            status |= STATUS_CUT                       # (every walker of that track is cut)
        if not on_track[i]:
            status |= STATUS_LINK
            size_ratio[i] = 1.0

    # size and centre
    size_wlh = prior[cls].copy()
    size_src = np.zeros(M, np.int32)
    size_placed = box[:, :2].copy()
    sized = member & (psrc != 0)
    with np.errstate(invalid="ignore", over="ignore"):
        ln_new, wd_new = size_ratio[:, 0] * len0, size_ratio[:, 1] * wid0
        size_wlh[sized, 0], size_wlh[sized, 1] = wd_new[sized], ln_new[sized]
        size_src[sized] = (pooled[sized, 0] * SRC_LENGTH) | (pooled[sized, 1] * SRC_WIDTH)
        fr = np.where(member, frame, 0)
        sx, sy = (np.zeros(M), np.zeros(M)) if ego is None else (ego[fr, 0], ego[fr, 1])
        cx, cy, a, b, hc, hs = (rect[:, k_] for k_ in range(6))
        take = sized & np.isfinite(sx) & np.isfinite(sy) & np.isfinite(rect).all(1)
        ex, ey = sx - cx, sy - cy
        pu, pv = (ex * hc) + (ey * hs), (ey * hc) - (ex * hs)
        su, sv = np.where(pu >= 0.0, 1.0, -1.0), np.where(pv >= 0.0, 1.0, -1.0)
        au, av = b >= thin, a >= thin
        du = np.where(au, su * ((a - ln_new) * 0.5), 0.0)
        dv = np.where(av, sv * ((b - wd_new) * 0.5), 0.0)
        x = ((du * hc) - (dv * hs)) + cx
        y = ((du * hs) + (dv * hc)) + cy
    box[take, 0], box[take, 1] = x[take], y[take]

    # velocity on the new centres
    size_vel = np.zeros((M, 2), np.float64)
    Wc = min(W, F)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for i in np.flatnonzero(member):
            if W == 0:
                n_, p_ = int(vnext[i]), int(vprev[i])
                tp = t[n_] if n_ >= 0 else t[i]
                tm = t[p_] if p_ >= 0 else t[i]
                if n_ >= 0 and p_ >= 0 and tp - tm <= max_dt:
                    size_vel[i] = (box[n_, :2] - box[p_, :2]) / (tp - tm)
                elif n_ >= 0 and tp - t[i] <= max_dt:
                    size_vel[i] = (box[n_, :2] - box[i, :2]) / (tp - t[i])
                elif p_ >= 0 and t[i] - tm <= max_dt:
                    size_vel[i] = (box[i, :2] - box[p_, :2]) / (t[i] - tm)
                continue
            back, ahead = min(int(pos[i]), Wc), min(int(ln[i]) - 1 - int(pos[i]), Wc)
            want = back + 1 + ahead
            if want > F:
                want, status = F, status | STATUS_CUT
            m = int(i)
            for _ in range(back):
                if vprev[m] < 0:
                    break
                m = int(vprev[m])
            win = []
            while len(win) < want and m >= 0:
                win.append(m)
                m = int(vnext[m])
            n = len(win)
            if n < 2:
                continue
            St = Stt = Sx = Sy = Stx = Sty = np.float64(0.0)
            for j in win:
                tj, xj, yj = t[j] - t[i], box[j, 0] - box[i, 0], box[j, 1] - box[i, 1]
                St, Stt, Sx, Sy, Stx, Sty = St + tj, Stt + (tj * tj), Sx + xj, Sy + yj, Stx + (tj * xj), Sty + (tj * yj)
            dn = np.float64(n)
            den = (dn * Stt) - (St * St)
            if den > 0.0:
                size_vel[i] = ((dn * Stx) - (St * Sx)) / den, ((dn * Sty) - (St * Sy)) / den
    return dict(box=box, flags=flags, size_wlh=size_wlh, size_src=size_src, size_ratio=size_ratio, size_obs=size_obs,
                size_placed=size_placed, size_vel=size_vel, status=int(status))
