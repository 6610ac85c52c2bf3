"""Cases of the point ownership (cm3d_amd.pointowner; cm3d_point_owner) and an independent brute-force statement of the rule: per frame,
a dictionary from point to the sorted list of its claimants, and the claimant that beats all the others by the pairwise rule as the
header words it.  The crafted cases are the smallest shapes at which the kernels can go wrong: lists that end at, one before and one
behind a wave (64) and a workgroup pass (256) and several passes (1024); frames of up to CM3D_MAX_MASKS_PER_FRAME masks that all claim
the same points; ties of score and length, NaN scores; the MIN_KEEP threshold; frames that share point numbers, a frame without masks,
the first and the last point of a frame and the numbers just outside.  A case is a dict: P, mask_off, hit_off, hit_idx, hit_xyz, score
and `runs`, a list of (rule, min_keep)."""
import numpy as np

MEDOID_TILE = 64
SEAM_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
CLAIMANT_COUNTS = (2, 33, 64, 65, 1024)
BOTH = [("score", 1), ("smallest", 1), ("score", 5), ("smallest", 5)]
N_RANDOM = 200


def make(name, P, frames, runs=BOTH):
    """frames: a list of frames, each a list of (score, [point indices]) in mask order."""
    mask_off, hit_off, idx, score = [0], [0], [], []
    for fr in frames:
        for s, pts in fr:
            idx.extend(int(p) for p in pts)
            hit_off.append(len(idx))
            score.append(float(s))
        mask_off.append(len(score))
    idx = np.asarray(idx, np.int32).reshape(-1)
    m_of = np.repeat(np.arange(len(score)), np.diff(hit_off)).astype(np.float32)
    xyz = np.stack([idx.astype(np.float32), m_of, np.arange(idx.size, dtype=np.float32) * 0.25, np.zeros(idx.size, np.float32)], 1)
    return dict(name=name, P=int(P), mask_off=np.asarray(mask_off, np.int32), hit_off=np.asarray(hit_off, np.int32), hit_idx=idx,
                hit_xyz=np.ascontiguousarray(xyz, np.float32).reshape(-1, 4), score=np.asarray(score, np.float64), runs=list(runs))


def seam_cases():
    out = []
    for n in SEAM_SIZES:
        B = [3 * j + 1 for j in range(n)]
        A = B[::2]
        # B has the higher score and the longer list: the rules disagree on every point of A
        out.append(make(f"seam_{n}", 3 * n + 2, [[(0.4, A), (0.9, B)]]))
    out.append(make("seam_257_b_first", 3 * 257 + 2, [[(0.9, [3 * j + 1 for j in range(257)]), (0.4, [3 * j + 1 for j in range(0, 257, 2)])]]))
    return out


def claimant_cases():
    out = []
    for n in CLAIMANT_COUNTS:
        fr = [(round(((k * 37) % 11) / 10.0, 2), [5, 6, 7, 10 + k] if k % 3 else [10 + k, 5, 6, 7]) for k in range(n)]
        out.append(make(f"claimants_{n}", n + 12, [fr], [("score", 1), ("smallest", 1), ("score", 2)]))
    return out


def tie_cases():
    nan = float("nan")
    return [
        make("tie_score_and_length", 40, [[(0.5, [1, 2, 3, 4]), (0.5, [3, 4, 5, 6]), (0.5, [6, 1, 9, 4])]]),
        make("tie_score_only", 40, [[(0.5, [1, 2, 3, 4, 5, 6]), (0.5, [3, 4, 5]), (0.5, [5, 6, 7, 8])]]),
        make("nan_score", 40, [[(nan, [1, 2, 3]), (0.1, [2, 3, 4, 5]), (-1.0, [1, 5, 6])]]),
        make("two_nan_scores", 40, [[(nan, [1, 2, 3, 4]), (nan, [2, 3, 4]), (nan, [1, 2, 3, 9]), (0.0, [9, 10])]]),
        make("inf_scores", 40, [[(float("-inf"), [1, 2, 3]), (nan, [1, 2, 3, 4]), (float("inf"), [3, 4]), (-0.0, [1, 4, 8]), (0.0, [1, 4, 8])]]),
    ]


def min_keep_cases():
    K = 5
    shared = list(range(100, 140))
    out = []
    for own in (K - 1, K):                      # the loser keeps K - 1 (kept whole) or K (stripped) positions
        loser = list(range(own)) + shared[:7]
        out.append(make(f"min_keep_kept_{own}", 200, [[(0.2, loser), (0.9, shared)]], [("score", K), ("score", K + 1), ("score", 1)]))
    out.append(make("min_keep_1_wholly_owned", 200, [[(0.2, shared[3:9]), (0.9, shared)]], [("score", 1), ("smallest", 1)]))
    return out


def frame_cases():
    P = 50
    return [
        make("same_point_in_two_frames", P, [[(0.9, [1, 2, 3]), (0.1, [2, 3, 4])], [(0.1, [1, 2, 3]), (0.9, [3, 4])]]),
        make("empty_frame_between", P, [[(0.9, [1, 2, 3]), (0.1, [2, 3, 4])], [], [(0.3, [2, 3]), (0.9, [3, 4]), (0.5, [])], []]),
        make("first_and_last_point", P, [[(0.9, [0, 7, P - 1]), (0.1, [0, P - 1])], [(0.2, [P - 1, 0]), (0.1, [0, 3, P - 1])]]),
        make("outside_the_frame", P, [[(0.9, [-1, 7, P, 8]), (0.1, [-1, P, 8, 2 ** 31 - 1, -2 ** 31])], [(0.5, [P, -1, P + 1])]]),
        make("no_points_per_frame", 0, [[(0.9, [0, 1, 2]), (0.1, [0, 1])]]),
    ]


def crafted():
    return seam_cases() + claimant_cases() + tie_cases() + min_keep_cases() + frame_cases()


def random_case(seed):
    rng = np.random.default_rng(9000 + seed)
    F, P = int(rng.integers(1, 5)), int(rng.integers(1, 501))
    frames = []
    for _ in range(F):
        fr = []
        for _ in range(int(rng.integers(0, 41))):
            n = int(min(P, rng.integers(0, 2 + int(rng.integers(1, 61)))))
            centre = int(rng.integers(0, P))             # lists of a frame crowd the same stretch of the cloud: they overlap
            pool = np.unique(np.clip(centre + rng.integers(-40, 41, size=3 * n + 1), 0, P - 1))
            pts = np.sort(rng.choice(pool, size=min(n, pool.size), replace=False))
            s = round(float(rng.integers(0, 12)) / 10.0, 2) if rng.random() > 0.03 else float("nan")
            fr.append((s, pts.tolist()))
        frames.append(fr)
    rule = ("score", "smallest")[seed % 2]
    return make(f"random_{seed}", P, frames, [(rule, int(rng.integers(1, 7)))])


def random_cases():
    return [random_case(s) for s in range(N_RANDOM)]


# ---- the brute-force statement --------------------------------------------------------------------------------------------------
def beats(rule, sa, na, a, sb, nb, b):
    """a beats b, word for word: a NaN score is lower than every number, two NaNs are equal."""
    a_nan, b_nan = sa != sa, sb != sb
    higher = (not a_nan) and (b_nan or sa > sb)
    same = (a_nan and b_nan) or sa == sb
    if rule == "score":
        return higher or (same and na < nb) or (same and na == nb and a < b)
    return na < nb or (na == nb and higher) or (na == nb and same and a < b)


def clamp_lists(hit_off, cap):
    off = [int(v) for v in hit_off]
    out = []
    for m in range(len(off) - 1):
        lo = min(max(off[m], 0), cap)
        hi = min(max(off[m + 1], lo), cap)
        out.append((lo, hi))
    return out


def brute(case, rule, min_keep, idx_cap=None, hit_off=None):
    """The result of the stage on a case by brute force: dict(ow_owner, keep, ow_off, ow_tile_off, ow_status, ow_lost, claims) with
    claims a dict (frame, point) -> the sorted list of the masks that list it."""
    idx, score, P = case["hit_idx"], case["score"], case["P"]
    cap = len(idx) if idx_cap is None else idx_cap
    lists = clamp_lists(case["hit_off"] if hit_off is None else hit_off, cap)
    M = len(lists)
    n = [hi - lo for lo, hi in lists]
    end = lists[-1][1] if M else 0
    owner = [0] * end
    claims = {}
    mo = case["mask_off"]
    frame_of = {}
    for f in range(len(mo) - 1):
        for m in range(int(mo[f]), int(mo[f + 1])):
            frame_of[m] = f
            for i in range(*lists[m]):
                p = int(idx[i])
                if 0 <= p < P:
                    c = claims.setdefault((f, p), [])
                    if m not in c:
                        c.append(m)
    for c in claims.values():
        c.sort()
    wins = lambda a, b: beats(rule, score[a], n[a], a, score[b], n[b], b)
    owner_of = {}
    for key, c in claims.items():               # the claimant that beats all the others: a candidate by one walk, then held against each
        best = c[0]
        for b in c[1:]:
            if wins(b, best):
                best = b
        assert all(a == best or (wins(best, a) and not wins(a, best)) for a in c), key
        owner_of[key] = best
    for m in range(M):
        for i in range(*lists[m]):
            p = int(idx[i])
            owner[i] = owner_of[frame_of[m], p] if 0 <= p < P else m
    keep, status, lost, cnt = [False] * end, [], [], []
    for m, (lo, hi) in enumerate(lists):
        mine = [owner[i] == m for i in range(lo, hi)]
        if hi == lo:
            status.append(2), lost.append(0), cnt.append(0)
        elif sum(mine) < min_keep:
            keep[lo:hi] = [True] * (hi - lo)
            status.append(1), lost.append(0), cnt.append(hi - lo)
        else:
            keep[lo:hi] = mine
            status.append(0), lost.append(hi - lo - sum(mine)), cnt.append(sum(mine))
    cnt = np.asarray(cnt, np.int64)
    return dict(ow_owner=np.asarray(owner, np.int32).reshape(-1), keep=np.asarray(keep, bool).reshape(-1),
                ow_off=np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32),
                ow_tile_off=np.concatenate([[0], np.cumsum((cnt + MEDOID_TILE - 1) // MEDOID_TILE)]).astype(np.int32),
                ow_status=np.asarray(status, np.int32).reshape(-1), ow_lost=np.asarray(lost, np.int32).reshape(-1), claims=claims)


def host(case, rule, min_keep, idx_cap=None, hit_off=None):
    """The host statement's result on a case, with the lists it keeps: ow_idx, ow_xyz."""
    from cm3d_amd import pointowner as po
    off = case["hit_off"] if hit_off is None else hit_off
    res = po.point_owner_host(case["hit_idx"], off, case["mask_off"], case["score"], case["P"], rule, min_keep, idx_cap)
    res["ow_idx"], res["ow_xyz"] = po.owned_lists(case["hit_idx"], case["hit_xyz"], off, res, idx_cap)
    return res


RESULT_KEYS = ("ow_owner", "keep", "ow_off", "ow_tile_off", "ow_status", "ow_lost")


def assert_same(got, exp, what, keys=RESULT_KEYS):
    for k in keys:
        g, e = np.asarray(got[k]), np.asarray(exp[k])
        assert g.shape == e.shape and np.array_equal(g, e), (what, k, np.flatnonzero(g.reshape(-1)[:e.size] != e.reshape(-1)[:g.size])[:8])
