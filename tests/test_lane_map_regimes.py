"""CPU: the city-scale lane maps and crafted centroids of tests/lane_maps.py really reach the regimes of the lane
search that tests/test_gpu_stage2.py is meant to exercise (grown cells, crowded cells, far rings, the exact-scan
fallback, exact ties).  Without these checks a generator change could quietly send every GPU case back to the 4 m
grid of the small synthetic tables."""
import numpy as np
import pytest

from tests import lane_maps as lm


def _dist64(cent, lane):
    """float64 distances (K, L) of float32 centroids to float32 lane points, the reference's cdist arithmetic."""
    c = np.asarray(cent, np.float32)[:, :2].astype(np.float64)
    p = np.asarray(lane, np.float64).astype(np.float32)[:, :2].astype(np.float64)
    return np.sqrt((c[:, 0, None] - p[None, :, 0]) ** 2 + (c[:, 1, None] - p[None, :, 1]) ** 2)


def _min_and_ties(cent, lane, chunk=8):
    """Per centroid: the float64 minimum distance and how many lane points attain it."""
    mins, counts = [], []
    for a in range(0, cent.shape[0], chunk):
        d = _dist64(cent[a:a + chunk], lane)
        m = d.min(1)
        mins.append(m)
        counts.append((d == m[:, None]).sum(1))
    return np.concatenate(mins), np.concatenate(counts)


@pytest.fixture(scope="module")
def maps():
    return lm.city_maps()


@pytest.mark.parametrize("k", range(5))
def test_city_map_reaches_the_grown_grid(maps, k):
    m = maps[k]
    L = m.lane.shape[0]
    assert 2e5 <= L <= 6e5, L
    ext = np.ptp(m.lane[:, :2], 0)
    assert 1400 <= ext.min() and ext.max() <= 4100, ext
    lo, hi = m.lane[:, :2].min(0), m.lane[:, :2].max(0)
    if k < 4:
        assert lo.min() < 100 and hi.max() > 1900, (lo, hi)          # from near the origin out to km, like a map frame
    else:
        assert np.hypot(*hi) > 10000, hi                             # the copy out at ~10 km
    x0, y0, h, inv_h, gw, gh = lm.grid_geometry(m.lane)
    assert h > lm.LG_CELL0 and gw * gh <= lm.LG_MAX_CELLS and gw % 2 == 1
    cc = lm.cell_counts(m.lane)
    assert cc.sum() == L
    # crowded cells are the rule, not an accident: the biggest holds many times the whole-wave threshold
    assert cc.max() > 10 * lm.LG_BIG_CELL and (cc > lm.LG_BIG_CELL).sum() > 1000, (cc.max(), (cc > lm.LG_BIG_CELL).sum())
    # and the park leaves a hole of many empty cells in a row
    px0, py0, px1, py1 = m.park
    assert not ((m.lane[:, 0] > px0) & (m.lane[:, 0] < px1) & (m.lane[:, 1] > py0) & (m.lane[:, 1] < py1)).any()
    assert px1 - px0 > 300 and py1 - py0 > 300


@pytest.mark.parametrize("k", range(5))
def test_crafted_centroids_fall_where_they_are_meant_to(maps, k):
    m = maps[k]
    c = lm.crafted_centroids(m, seed=k)
    x0, y0, h, inv_h, gw, gh = lm.grid_geometry(m.lane)
    h = float(h)
    l32 = m.lane.astype(np.float32)
    # park: more than 2 h from every lane point (the search needs rings beyond the first batch)
    dmin, _ = _min_and_ties(c["park"], m.lane, chunk=16)
    assert dmin.min() > 2 * h, (dmin.min(), h)
    # fallback: more than 64 h outside the bounding box, so far out in the kernel's own cell arithmetic that the ring
    # search starts beyond LG_MAX_RINGS and goes straight to the exact scan
    bb_lo, bb_hi = l32[:, :2].min(0).astype(np.float64), l32[:, :2].max(0).astype(np.float64)
    p = c["fallback"][:, :2].astype(np.float64)
    gap = np.maximum(np.maximum(bb_lo - p, p - bb_hi), 0).max(1)
    assert gap.min() > lm.LG_MAX_RINGS * h, (gap.min(), h)
    qi = np.floor((p[:, 0] - float(x0)) * float(inv_h))
    qj = np.floor((p[:, 1] - float(y0)) * float(inv_h))
    out = np.maximum(np.where(qi < 0, -qi, np.where(qi >= gw, qi - gw + 1, 0)), np.where(qj < 0, -qj, np.where(qj >= gh, qj - gh + 1, 0)))
    assert (out - 1 >= lm.LG_MAX_RINGS).all()
    p = c["far"][:, :2].astype(np.float64)
    gap = np.maximum(np.maximum(bb_lo - p, p - bb_hi), 0).max(1)
    assert (gap > 9 * h).all() and (gap < lm.LG_MAX_RINGS * h).all()
    # ties: the minimum distance is attained by two or more lane points, exactly, in float64
    dmin, n_at_min = _min_and_ties(c["tie"], m.lane)
    assert c["tie"].shape[0] >= 150 and (n_at_min >= 2).all(), np.flatnonzero(n_at_min < 2)
    assert (n_at_min >= 4).sum() >= 30                 # the quarter-metre offsets on the centre line: four at once
    # near: within 5 m; on: distance 0, duplicated rows among them
    dmin, n_at_min = _min_and_ties(c["near"], m.lane, chunk=16)
    assert dmin.max() <= 5.0 + 1e-3
    dmin, n_at_min = _min_and_ties(c["on"], m.lane, chunk=16)
    assert (dmin == 0).all() and (n_at_min >= 2).sum() >= 20
    # cell boundaries: the five ulp-variants of a boundary do not all land in one cell of the kernel's centroid binning
    cb = c["cell"][:, :2].astype(np.float64).reshape(-1, 5, 2)
    ci = np.floor((cb[..., 0] - float(x0)) * float(inv_h))
    cj = np.floor((cb[..., 1] - float(y0)) * float(inv_h))
    split = (np.ptp(ci, 1) > 0) | (np.ptp(cj, 1) > 0)
    assert split.mean() > 0.8, split.mean()
    # junction centroids sit in cells that are crowded
    cc = lm.cell_counts(m.lane)
    jx = np.clip(np.floor((c["junction"][:, 0] - x0) * inv_h).astype(int), 0, gw - 1)
    jy = np.clip(np.floor((c["junction"][:, 1] - y0) * inv_h).astype(int), 0, gh - 1)
    assert np.median(cc[jy, jx]) > 4 * lm.LG_BIG_CELL


def test_degenerate_tables_are_what_they_say():
    t = dict(lm.degenerate_tables())
    assert t["one"].shape[0] == 1 and t["two"].shape[0] == 2
    assert lm.grid_geometry(t["hline"])[5] == 1 and lm.grid_geometry(t["vline"])[4] == 1
    g = lm.grid_geometry(t["same"])
    assert g[4] == 1 and g[5] == 1
    d = t["dups"][:, :2]
    assert np.unique(d, axis=0).shape[0] < d.shape[0] // 2


def test_margin_cases_need_the_margin():
    """lane_maps.margin_cases: on every table the emulated search with the ring-stop margin returns the brute force's
    index and the one without it does not; the cases cover several stop rings and grown cell sizes."""
    cases = lm.margin_cases()
    assert len(cases) >= 10
    assert {R for _, _, R in cases} >= {5, 9, 15, 24}
    assert len({float(lm.grid_geometry(t)[2]) for t, _, _ in cases}) >= 2
    for t, c, R in cases:
        x0, y0, h, inv_h, gw, gh = lm.grid_geometry(t)
        assert h > lm.LG_CELL0
        d = _dist64(c[None], t)[0]
        j = int(np.argmin(d))
        assert lm.emulate_lane_nn(t, c, use_margin=True) == j
        assert lm.emulate_lane_nn(t, c, use_margin=False) != j
        assert d[j] < R * float(h) and np.sort(d)[1] < R * float(h)      # both points within R h: only the margin tells them apart
