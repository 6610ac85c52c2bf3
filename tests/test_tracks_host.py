"""CPU: the host statement of the box track stage (cm3d_amd.tracks.box_tracks_host, the rule of include/cm3d_hip.h's cm3d_box_tracks)
against a separately written scalar loop and closed-form answers on tests/tracks_cases.py; the velocity stage's own output sets no
status bit; the switch is off at its defaults; the entry points' flags are errors without --velocity track."""
import argparse
import math

import numpy as np
import pytest

from cm3d_amd import tracks as T
from cm3d_amd import velocity as V
from tests import tracks_cases as tc
from tests import velocity_cases as vc

CASES = tc.all_cases()
RUNS = [(c, st) for c in CASES for st in c["settings"]]
RUN_IDS = [f"{c['name']}-{st[0]}-{st[1]}-{st[2]}" for c, st in RUNS]
INT_KEYS = ("track_id", "track_pos", "track_len", "flags")
F64_KEYS = ("track_stat", "vel_smooth", "box")


# ------------------------------------------------------------------------------------------------ the scalar loop
def _plain(box, flags, mask_frame, next_match, prev_match, frame_time, min_length, score, W):
    """The rule mask by mask, Python floats and lists: every mask finds its own head by walking back, walks its whole track for the
    statistics and collects its window by position; nothing is shared between masks."""
    box, flags, frame = box.tolist(), flags.tolist(), mask_frame.tolist()
    nm, pm, time = next_match.tolist(), prev_match.tolist(), frame_time.tolist()
    M, F = len(flags), len(time)
    status = 0

    def kept(i):
        return (flags[i] & 3) == 3 and 0 <= frame[i] < F

    def t_of(i):
        return time[frame[i]]

    def link(i, fwd, note=False):
        """The valid next (fwd) or previous link of kept mask i, or -1; note: record the status bits."""
        nonlocal status
        j = nm[i] if fwd else pm[i]
        if j < -1 or j >= M:
            status |= 2 if note else 0
            return -1
        if j < 0:
            return -1
        back = pm[j] if fwd else nm[j]
        ok = kept(j) and back == i and (t_of(j) > t_of(i) if fwd else t_of(j) < t_of(i))
        if not ok:
            status |= 4 if note else 0
            return -1
        return j

    out = dict(track_id=[-1] * M, track_pos=[-1] * M, track_len=[0] * M, track_stat=[[0.0] * 4 for _ in range(M)],
               vel_smooth=[[0.0, 0.0] for _ in range(M)], box=[row[:] for row in box], flags=flags[:])
    for i in range(M):
        if (flags[i] & 3) == 3 and not 0 <= frame[i] < F:
            status |= 1
        if not kept(i):
            continue
        link(i, True, note=True)
        link(i, False, note=True)
        head, p = i, 0
        while link(head, False) >= 0:
            head, p = link(head, False), p + 1
        track = [head]
        while link(track[-1], True) >= 0:
            track.append(link(track[-1], True))
        L = len(track)
        total, top = 0.0, box[head][7]
        for m in track:
            total = total + box[m][7]
            top = box[m][7] if box[m][7] > top else top
        dx, dy = box[track[-1]][0] - box[head][0], box[track[-1]][1] - box[head][1]
        out["track_id"][i], out["track_pos"][i], out["track_len"][i] = head, p, L
        out["track_stat"][i] = [total, top, t_of(track[-1]) - t_of(head), math.sqrt((dx * dx) + (dy * dy))]
        if W > 0:
            win = [track[q] for q in range(L) if p - W <= q <= p + W]
            n = len(win)
            if n >= 2:
                St = Stt = Sx = Sy = Stx = Sty = 0.0
                for j in win:
                    t, x, y = t_of(j) - t_of(i), box[j][0] - box[i][0], box[j][1] - box[i][1]
                    St = St + t; Stt = Stt + (t * t); Sx = Sx + x; Sy = Sy + y; Stx = Stx + (t * x); Sty = Sty + (t * y)
                den = (float(n) * Stt) - (St * St)
                if den > 0.0:
                    out["vel_smooth"][i] = [((float(n) * Stx) - (St * Sx)) / den, ((float(n) * Sty) - (St * Sy)) / den]
        if score == "mean":
            out["box"][i][7] = total / float(L)
        elif score == "max":
            out["box"][i][7] = top
        if L < min_length:
            out["flags"][i] = flags[i] & ~2
            out["box"][i][9] = float(out["flags"][i])
    res = {k: np.array(out[k], np.int32).reshape(M) for k in INT_KEYS}
    res.update(track_stat=np.array(out["track_stat"], np.float64).reshape(M, 4), vel_smooth=np.array(out["vel_smooth"], np.float64).reshape(M, 2),
               box=np.array(out["box"], np.float64).reshape(M, tc.BOX_STRIDE), status=status)
    return res


def _assert_same(got, exp, what=""):
    for k in INT_KEYS:
        assert np.array_equal(got[k], exp[k]), (what, k)
    for k in F64_KEYS:
        assert got[k].tobytes() == exp[k].tobytes(), (what, k)


@pytest.mark.parametrize("case,st", RUNS, ids=RUN_IDS)
def test_statement_equals_the_scalar_loop(case, st):
    got, exp = T.box_tracks_host(*tc.args_of(case), *st), _plain(*tc.args_of(case), *st)
    _assert_same(got, exp)
    assert got["status"] == exp["status"] == case["status"]


def test_pinned_answers():
    n = sum(tc.check_pinned(c, st, T.box_tracks_host(*tc.args_of(c), *st)) for c, st in RUNS)
    assert n >= 18


def test_dyadic_scene_is_exact_for_every_window():
    """The prototype's scene: ids, lengths, the filter and (2.0, -1.0) exactly at W = 1, 2 and 3; the box that shows once is what
    min_length = 2 removes beside nothing else of its frame."""
    c = tc.by_name("dyadic_constant_velocity")
    once = c["expect"][tc.DEFAULT]["once"]
    for W in (1, 2, 3):
        got = T.box_tracks_host(*tc.args_of(c), 2, "own", W)
        moving = got["track_len"] >= 2
        assert moving.sum() == 29 and (got["vel_smooth"][moving] == np.array(tc.DYADIC_V)).all() and not got["vel_smooth"][~moving].any()
        assert got["track_len"][once] == 1 and got["flags"][once] == 1 and got["box"][once, 9] == 1.0
        changed = np.flatnonzero(got["flags"] != c["flags"])
        assert changed.tolist() == [once]
        assert np.array_equal(np.delete(got["box"], once, 0), np.delete(c["box"], once, 0))


def test_sum_is_taken_in_track_order():
    c = tc.by_name("frames_out_of_time_order")
    got = T.box_tracks_host(*tc.args_of(c))
    assert got["track_stat"][0, 0] == 1.0 and float(np.sum(c["box"][:4, 7])) != 1.0 and sum(c["box"][:4, 7].tolist()) == 2.0


@pytest.mark.parametrize("case", [c for c in CASES if c["fixed"] is not None], ids=lambda c: c["name"])
def test_a_status_case_changes_only_what_the_rule_says(case):
    """The outputs are those of the case with the offending entry read as the rule reads it; the in/out arrays differ only where the
    case itself differs from it."""
    for st in case["settings"]:
        bad, good = T.box_tracks_host(*tc.args_of(case), *st), T.box_tracks_host(*tc.args_of(case["fixed"]), *st)
        assert bad["status"] == case["status"] and good["status"] == 0
        for k in ("track_id", "track_pos", "track_len", "track_stat", "vel_smooth"):
            assert bad[k].tobytes() == good[k].tobytes(), k
        same = case["flags"] == case["fixed"]["flags"]
        assert np.array_equal(bad["flags"][same], good["flags"][same]) and np.array_equal(bad["box"][same], good["box"][same])
        assert np.array_equal(bad["flags"][~same], case["flags"][~same]) and np.array_equal(bad["box"][~same], case["box"][~same])


@pytest.mark.parametrize("name", ["three_link_chain", "constant_velocity", "middle_frame_not_kept", "global_magnitude", "two_scenes"])
def test_velocity_stage_output_sets_no_status_bit(name):
    """What cm3d_box_velocity leaves (its host statement on a velocity case) is mutual, between kept boxes and forward in time."""
    c = vc.by_name(name)
    vel = V.track_velocity_host(*vc.args_of(c))
    frame = np.repeat(np.arange(len(c["mask_off"]) - 1), np.diff(c["mask_off"]))
    got = T.box_tracks_host(c["box"], c["flags"], frame, vel["next_match"], vel["prev_match"], c["frame_time"], 2, "mean", 2)
    assert got["status"] == 0 and vel["status"] == 0
    linked = vel["next_match"] >= 0
    assert linked.any() and (got["track_len"][linked] >= 2).all()
    assert np.array_equal(got["track_pos"][vel["next_match"][linked]], got["track_pos"][linked] + 1)
    if name == "three_link_chain":
        assert got["track_len"].max() == 4


def test_defaults_are_off_and_arguments_are_checked():
    assert not T.Tracks().active and not T.Tracks(1, "own", 0).active
    assert T.Tracks(2).active and T.Tracks(score="mean").active and T.Tracks(score="max").active and T.Tracks(smooth_window=1).active
    assert [T.Tracks(score=s).score_mode for s in T.SCORE_MODES] == [0, 1, 2]
    for bad in (dict(min_length=0), dict(smooth_window=-1), dict(score="median")):
        with pytest.raises(ValueError):
            T.Tracks(**bad)


def _parser():
    ap = argparse.ArgumentParser()
    V.add_arguments(ap)
    T.add_arguments(ap)
    return ap


@pytest.mark.parametrize("flag", [["--track-min-length", "2"], ["--track-score", "mean"], ["--velocity-smooth", "1"]])
def test_a_flag_without_velocity_track_is_an_argparse_error(flag, capsys):
    ap = _parser()
    with pytest.raises(SystemExit) as e:
        T.from_args(ap.parse_args(flag), ap)
    assert e.value.code == 2 and "--velocity track" in capsys.readouterr().err
    with pytest.raises(ValueError):
        T.from_args(ap.parse_args(flag))
    tr = T.from_args(ap.parse_args(["--velocity", "track"] + flag), ap)
    assert tr is not None and tr.active


def test_flags_at_their_defaults_give_no_stage():
    ap = _parser()
    assert T.from_args(ap.parse_args([]), ap) is None
    assert T.from_args(ap.parse_args(["--velocity", "track", "--track-min-length", "1", "--track-score", "own", "--velocity-smooth", "0"]), ap) is None
    with pytest.raises(SystemExit):
        T.from_args(ap.parse_args(["--velocity", "track", "--track-min-length", "0"]), ap)
    tr = T.from_args(ap.parse_args(["--velocity", "track", "--track-min-length", "3", "--track-score", "max", "--velocity-smooth", "2"]), ap)
    assert (tr.min_length, tr.score, tr.smooth_window) == (3, "max", 2)
