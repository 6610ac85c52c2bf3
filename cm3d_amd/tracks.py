"""Host side of the box track stage (include/cm3d_hip.h: cm3d_box_tracks; the call behind cm3d_box_velocity).

The velocity stage (cm3d_amd.velocity) associates the kept boxes of consecutive keyframes and leaves two pointer arrays on the device,
next_match and prev_match.  This stage follows them: every kept box gets the id, position and length of its track, a track carries four
statistics, a box can take its track's mean or greatest score, a box of a short track can be dropped, and a velocity can be taken as
the least-squares slope over a window of the track instead of the three-point difference.  This module is the rule's statement to the
bit (box_tracks_host), the switches of an engine (Tracks) and the flags of the entry points.  Nothing here is tuned, and what the stage
does to label quality has not been measured.
"""
from dataclasses import dataclass

import numpy as np

from ._lib import BOX_STRIDE

SCORE_MODES = ("own", "mean", "max")                 # score_mode 0, 1, 2 of cm3d_box_tracks
STATUS_FRAME, STATUS_RANGE, STATUS_LINK = 1, 2, 4    # a kept mask's frame outside the batch; a match outside [-1, M); a link that is not one


def score_code(score):
    if score not in SCORE_MODES:
        raise ValueError(f"score: one of {SCORE_MODES}, not {score!r}")
    return SCORE_MODES.index(score)


@dataclass
class Tracks:
    """The opt-in track stage of a LiftEngine with Velocity(...): behind the velocity call, cm3d_box_tracks follows next_match /
    prev_match.  min_length: a kept box whose track has fewer boxes loses its keep bit (1: no filter).  score: "own" leaves a box's
    score alone, "mean" / "max" write the mean / the greatest score of its track.  smooth_window W: the velocity of a box becomes the
    least-squares slope of the centres over the W boxes on either side of it in its track (0: the velocity stage's own).  At the
    defaults the stage is off: no buffer, no call.  None of the defaults is tuned."""
    min_length: int = 1
    score: str = "own"
    smooth_window: int = 0

    def __post_init__(self):
        self.min_length, self.smooth_window = int(self.min_length), int(self.smooth_window)
        if self.min_length < 1:
            raise ValueError("min_length >= 1")
        if self.smooth_window < 0:
            raise ValueError("smooth_window >= 0")
        score_code(self.score)

    @property
    def active(self):
        return self.min_length > 1 or self.score != "own" or self.smooth_window > 0

    @property
    def score_mode(self):
        return score_code(self.score)


def add_arguments(ap):
    """The three flags of the nuScenes entry points; at the defaults the output is that of --velocity track alone."""
    ap.add_argument("--track-min-length", type=int, default=1, metavar="N",
                    help="with --velocity track: drop a box whose track (the chain of its matches through the keyframes) holds fewer than N "
                         "boxes (default 1: none; untuned)")
    ap.add_argument("--track-score", choices=SCORE_MODES, default="own",
                    help="with --velocity track: a box's detection_score is its own, or the mean / the greatest of its track")
    ap.add_argument("--velocity-smooth", type=int, default=0, metavar="W",
                    help="with --velocity track: the velocity is the least-squares slope of the centres over W boxes on either side in the "
                         "track (default 0: the difference of the neighbouring matches)")


def from_args(args, ap=None):
    """Tracks from an entry point's flags; None at the defaults.  A flag away from its default without --velocity track is an error
    of the command line (ap.error when the parser is given, else ValueError)."""
    given = [flag for flag, off in (("--track-min-length", args.track_min_length == 1), ("--track-score", args.track_score == "own"),
                                    ("--velocity-smooth", args.velocity_smooth == 0)) if not off]
    try:
        if given and getattr(args, "velocity", "none") != "track":
            raise ValueError(f"{given[0]} needs --velocity track")
        tr = Tracks(args.track_min_length, args.track_score, args.velocity_smooth)
    except ValueError as e:
        if ap is None:
            raise
        ap.error(str(e))
    return tr if tr.active else None


def box_tracks_host(box, flags, mask_frame, next_match, prev_match, frame_time, min_length=1, score="own", smooth_window=0):
    """What cm3d_box_tracks computes (include/cm3d_hip.h states the rule), to the bit.  Returns a dict: track_id, track_pos, track_len
    (M,) int32, track_stat (M, 4) and vel_smooth (M, 2) float64 (zeros for smooth_window 0), the new box and flags (copies), status."""
    box = np.array(box, np.float64).reshape(-1, BOX_STRIDE)
    M = box.shape[0]
    flags = np.array(flags, np.int32).reshape(M)
    mask_frame = np.asarray(mask_frame, np.int64).reshape(M)
    nm, pm = np.asarray(next_match, np.int64).reshape(M), np.asarray(prev_match, np.int64).reshape(M)
    time = np.asarray(frame_time, np.float64).reshape(-1)
    F, W, mode = time.size, int(smooth_window), score_code(score)
    if F <= 0 or min_length < 1 or W < 0:
        raise ValueError("n_frames > 0, min_length >= 1, smooth_window >= 0")
    marked = (flags & 3) == 3
    in_frame = (mask_frame >= 0) & (mask_frame < F)
    kept = marked & in_frame
    status = STATUS_FRAME if (marked & ~in_frame).any() else 0
    t = np.where(kept, time[np.where(in_frame, mask_frame, 0)], 0.0)

    def valid(a, b, forward):
        """(a[i] where it is a valid link of kept i, else -1), status bits: b is the array that must point back."""
        out, bits = np.full(M, -1, np.int64), 0
        for i in np.flatnonzero(kept):
            j = int(a[i])
            if j < -1 or j >= M:
                bits |= STATUS_RANGE
            elif j >= 0:
                if kept[j] and b[j] == i and (t[j] > t[i] if forward else t[j] < t[i]):
                    out[i] = j
                else:
                    bits |= STATUS_LINK
        return out, bits
    vnext, b1 = valid(nm, pm, True)
    vprev, b2 = valid(pm, nm, False)
    status |= b1 | b2

    track_id, track_pos, track_len = np.full(M, -1, np.int32), np.full(M, -1, np.int32), np.zeros(M, np.int32)
    track_stat, vel_smooth = np.zeros((M, 4), np.float64), np.zeros((M, 2), np.float64)
    members = {}
    for h in np.flatnonzero(kept & (vprev < 0)):
        mem = [int(h)]
        while vnext[mem[-1]] >= 0:
            mem.append(int(vnext[mem[-1]]))
        members[int(h)] = mem
        total, top = np.float64(0.0), box[h, 7]
        for m in mem:
            total = total + box[m, 7]
            if box[m, 7] > top:
                top = box[m, 7]
        dx, dy = box[mem[-1], 0] - box[h, 0], box[mem[-1], 1] - box[h, 1]
        with np.errstate(invalid="ignore", over="ignore"):
            stat = [total, top, t[mem[-1]] - t[h], np.sqrt((dx * dx) + (dy * dy))]
        track_id[mem], track_pos[mem], track_len[mem], track_stat[mem] = h, np.arange(len(mem)), len(mem), stat
    if W > 0:
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            for mem in members.values():
                L = len(mem)
                for p, i in enumerate(mem):
                    win = mem[max(0, p - W):min(L - 1, p + W) + 1]
                    n = len(win)
                    if n < 2:
                        continue
                    St = Stt = Sx = Sy = Stx = Sty = np.float64(0.0)
                    for j in win:
                        tj, x, y = t[j] - t[i], box[j, 0] - box[i, 0], box[j, 1] - box[i, 1]
                        St, Stt, Sx, Sy, Stx, Sty = St + tj, Stt + (tj * tj), Sx + x, Sy + y, Stx + (tj * x), Sty + (tj * y)
                    dn = np.float64(n)
                    den = (dn * Stt) - (St * St)
                    if den > 0.0:
                        vel_smooth[i] = ((dn * Stx) - (St * Sx)) / den, ((dn * Sty) - (St * Sy)) / den
    new_box, new_flags = box.copy(), flags.copy()
    k = np.flatnonzero(kept)
    with np.errstate(invalid="ignore", over="ignore"):
        if mode == 1:
            new_box[k, 7] = track_stat[k, 0] / track_len[k].astype(np.float64)
        elif mode == 2:
            new_box[k, 7] = track_stat[k, 1]
    short = k[track_len[k] < int(min_length)]
    new_flags[short] &= ~np.int32(2)
    new_box[short, 9] = new_flags[short].astype(np.float64)
    return dict(track_id=track_id, track_pos=track_pos, track_len=track_len, track_stat=track_stat, vel_smooth=vel_smooth, box=new_box,
                flags=new_flags, status=int(status))
