"""The in-wave two-pass route of the medoid tile kernel (csrc/medoid.hip, md_inwave_tile): lists of 26 .. MD_INW_MAX points in
the scaled form get approximate column sums first and exact ones only for the columns that can be the tile's minimum.  Every list
here goes through cm3d_medoid2 with flags = 1 (the light instantiation, the product's call on the headline shape), all lists in ONE
batch per instantiation; expected positions come from the CPU oracle (orc_medoid: the reference's order -- direct form up to 25 points,
the expansion's fma chain, clamp_min_(0), sqrtf, ascending float32 sums, torch.argmin's "NaN counts as minimal, first wins"), never
from the library.  A call with colsum_opt (every exact column sum, the route switched off) is an extra cross-check."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INW_MAX = 256            # MD_INW_MAX: the longest list of the route (one stage of the wave's LDS slice)
N_MAX = 1.0e9            # MDA_N_MAX: squared norms from here on take the unscaled loop


def _cluster(rng, centre, n, spread):
    return (np.asarray(centre, np.float32) + rng.uniform(-spread, spread, (n, 3)).astype(np.float32)).astype(np.float32)


def _ring_with_centre_pair(rng, centre, n, ja, jb):
    """n points on a ring of 2-3 m around `centre`, and the SAME point, the centre, at positions ja and jb: two columns with identical
    terms, hence bit-identical sums, and the smallest ones -- the first must win."""
    ang = rng.uniform(0, 2 * np.pi, n)
    rad = rng.uniform(2.0, 3.0, n)
    p = np.stack([rad * np.cos(ang), rad * np.sin(ang), rng.uniform(-0.2, 0.2, n)], 1).astype(np.float32) + np.asarray(centre, np.float32)
    p = p.astype(np.float32)
    p[ja] = p[jb] = np.asarray(centre, np.float32)
    return p


def _cases():
    rng = np.random.default_rng(20261019)
    near = (620.0, 1480.0, 1.5)             # nuScenes' global frame
    cases = []
    for m in (26, 27, 63, 64, 65, 128, 129, 192, 193, INW_MAX, INW_MAX + 1):
        cases.append((f"len{m}", _cluster(rng, near, m, 2.5)))
    cases.append(("tie_in_tile", _ring_with_centre_pair(rng, near, 100, 10, 40)))
    cases.append(("tie_across_seam", _ring_with_centre_pair(rng, near, 100, 60, 70)))
    cases.append(("tie_across_seam_3_tiles", _ring_with_centre_pair(rng, near, 150, 63, 128)))
    cases.append(("identical_points", np.tile(np.asarray([near], np.float32), (100, 1))))
    cases.append(("identical_points_origin", np.zeros((70, 3), np.float32)))
    # many near-ties: the expansion's noise (an ulp of the squared norm) swallows distances of centimetres to metres
    for km, centre in (("1.7km", (1200.0, 1210.0, 2.0)), ("10km", (7000.0, 7140.0, 2.0)), ("30km", (21000.0, 21400.0, 2.0))):
        for m, spread in ((150, 0.3), (90, 3.0), (120, 0.05)):
            cases.append((f"cluster_{km}_{m}", _cluster(rng, centre, m, spread)))
    # a full group of candidates: the centre of a ring four times over
    p = _ring_with_centre_pair(rng, near, 120, 5, 77)
    p[33] = p[99] = p[5]
    cases.append(("tie_of_four", p))
    p = _cluster(rng, near, 80, 2.5)
    p[37, 1] = np.nan
    cases.append(("nan_coordinate", p))
    p = _cluster(rng, near, 80, 2.5)
    p[5, 0] = np.inf
    cases.append(("inf_coordinate", p))
    p = _cluster(rng, near, 130, 2.5)
    p[70, 2] = -np.inf
    cases.append(("neg_inf_coordinate_2_tiles", p))
    far = _cluster(rng, (40000.0, 30000.0, 2.0), 90, 3.0)                  # squared norms of 2.5e9: unscaled, today's loop
    assert ((far.astype(np.float64) ** 2).sum(1) > N_MAX).all()
    cases.append(("norm_above_n_max", far))
    mixed = _cluster(rng, (31140.0, 5500.0, 2.0), 100, 40.0)               # norms on both sides of MDA_N_MAX in one list
    n2 = (mixed.astype(np.float64) ** 2).sum(1)
    assert (n2 > N_MAX).any() and (n2 < N_MAX).any()
    cases.append(("norm_around_n_max", mixed))
    return cases


def _medoids(lists, indexed, colsum=False):
    """One call of cm3d_medoid2, flags = 1.  indexed: the gather form -- every list the rows of a frame cloud of its own, stored
    in a shuffled order and listed through hit_row."""
    import torch
    from cm3d_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda:0")
    Ms = [p.shape[0] for p in lists]
    n, tot = len(Ms), int(sum(Ms))
    off = np.concatenate([[0], np.cumsum(Ms)]).astype(np.int32)
    P4 = np.zeros((tot, 4), np.float32)
    rows = np.zeros(tot, np.int32)
    rng = np.random.default_rng(7)
    for k, p in enumerate(lists):
        if indexed:
            perm = rng.permutation(Ms[k]).astype(np.int32)                # list position i lives in cloud row perm[i]
            P4[off[k] + perm, :3] = p
            rows[off[k]:off[k + 1]] = perm
        else:
            P4[off[k]:off[k + 1], :3] = p
    tiles = (np.diff(off) + _lib.MEDOID_TILE - 1) // _lib.MEDOID_TILE
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    pts, hit_off, tile_off = t(P4), t(off), t(np.concatenate([[0], np.cumsum(tiles)]).astype(np.int32))
    pt_off, mask_frame, hit_row = t(off.copy()), t(np.arange(n, dtype=np.int32)), t(rows)
    med = torch.full((n,), -7, dtype=torch.int32, device=dev)
    cen = torch.full((n, 3), -7.0, dtype=torch.float32, device=dev)
    cs = torch.zeros(tot, dtype=torch.float32, device=dev) if colsum else None
    ws = torch.empty(int(L.cm3d_medoid_workspace_bytes(n, tot)), dtype=torch.uint8, device=dev)
    _lib.check(L.cm3d_medoid2(pts.data_ptr(), pt_off.data_ptr() if indexed else 0, mask_frame.data_ptr() if indexed else 0, n,
                              hit_off.data_ptr(), tile_off.data_ptr(), hit_row.data_ptr() if indexed else 0, tot, 0, med.data_ptr(),
                              cen.data_ptr(), cs.data_ptr() if colsum else 0, ws.data_ptr(), ws.numel(), 1, 0,
                              torch.cuda.current_stream().cuda_stream), "cm3d_medoid2")
    torch.cuda.synchronize()
    return med.cpu().numpy(), cen.cpu().numpy(), (cs.cpu().numpy() if colsum else None), off


@pytest.fixture(scope="module")
def world(oracle):
    cases = _cases()
    names = [c[0] for c in cases]
    lists = [c[1] for c in cases]
    exp, exp_cs = [], []
    for p in lists:
        P4 = np.zeros((p.shape[0], 4), np.float32)
        P4[:, :3] = p
        j, cs = oracle.medoid(P4, np.arange(p.shape[0], dtype=np.int32), want_colsum=True)
        exp.append(j)
        exp_cs.append(cs.copy())
    got = {indexed: _medoids(lists, indexed) for indexed in (False, True)}
    return dict(names=names, lists=lists, exp=np.asarray(exp, np.int32), exp_cs=exp_cs, got=got)


def _check(world, indexed, pick):
    med, cen, _, _ = world["got"][indexed]
    bad = []
    for k, name in enumerate(world["names"]):
        if not pick(name):
            continue
        e = int(world["exp"][k])
        want = world["lists"][k][e]
        if int(med[k]) != e or not np.array_equal(cen[k].view(np.uint32), want.view(np.uint32)):
            bad.append((name, int(med[k]), e))
    assert not bad, bad


def test_construction_of_the_cases(world):
    """The cases are what they claim to be (by the oracle's exact sums): the tied pair IS the minimum and the first of the pair
    wins, identical points give equal sums, the far clusters hold many exactly equal or zero terms, a NaN or inf coordinate makes
    every sum non-finite."""
    names, exp, cs = world["names"], world["exp"], world["exp_cs"]
    for name, first, second in (("tie_in_tile", 10, 40), ("tie_across_seam", 60, 70), ("tie_across_seam_3_tiles", 63, 128)):
        k = names.index(name)
        assert exp[k] == first and cs[k][first].view(np.uint32) == cs[k][second].view(np.uint32) and (np.delete(cs[k], [first, second]) > cs[k][first]).all()
    for name in ("identical_points", "identical_points_origin"):
        k = names.index(name)
        assert exp[k] == 0 and (cs[k] == cs[k][0]).all()
    for name in ("nan_coordinate", "inf_coordinate", "neg_inf_coordinate_2_tiles"):
        k = names.index(name)
        assert not np.isfinite(cs[k]).all() and np.isnan(cs[k]).any()
    k = names.index("tie_of_four")
    assert exp[k] == 5 and np.sum(cs[k].view(np.uint32) == cs[k][5].view(np.uint32)) == 4 and cs[k].min() == cs[k][5]
    k = names.index("cluster_30km_150")          # near-ties far beyond the group size: sums within the error bound of the smallest
    m = cs[k].size
    assert np.sum(cs[k] * (1 - 2 * (m + 2) * 2.0 ** -23) <= cs[k].min()) > 4


@pytest.mark.parametrize("indexed", [False, True], ids=["hit_xyz", "indexed"])
def test_list_lengths_and_the_route_s_limits(world, indexed):
    """26 / 27 (the direct form ends at 25), 63 / 64 / 65, 128 / 129 and 192 / 193 (tile seams), MD_INW_MAX = 256 and 257 (the route's
    limit: one stage of the wave's LDS slice; 257 points are a second stage and today's loop)."""
    _check(world, indexed, lambda n: n.startswith("len"))


@pytest.mark.parametrize("indexed", [False, True], ids=["hit_xyz", "indexed"])
def test_exact_ties_first_index_wins(world, indexed):
    _check(world, indexed, lambda n: n.startswith("tie_"))


@pytest.mark.parametrize("indexed", [False, True], ids=["hit_xyz", "indexed"])
def test_every_column_a_candidate_falls_back(world, indexed):
    """Identical points (all sums equal) and clusters 1.7 / 10 / 30 km out, where the expansion's cancellation leaves many zeros:
    more candidates than a group holds, the exact loop decides."""
    _check(world, indexed, lambda n: n.startswith("identical") or n.startswith("cluster_"))


@pytest.mark.parametrize("indexed", [False, True], ids=["hit_xyz", "indexed"])
def test_non_finite_coordinates_nan_counts_as_minimal(world, indexed):
    _check(world, indexed, lambda n: "nan" in n or "inf" in n)


@pytest.mark.parametrize("indexed", [False, True], ids=["hit_xyz", "indexed"])
def test_norms_above_the_scaled_form_s_limit(world, indexed):
    _check(world, indexed, lambda n: n.startswith("norm_"))


def test_exact_column_sums_agree_with_the_oracle_and_the_route(world):
    """Cross-check: with colsum_opt the route is off and every exact column sum comes back -- the oracle's bits on every list of
    finite points, and the same medoid as the in-wave route."""
    med, cen, cs, off = _medoids(world["lists"], False, colsum=True)
    for k, name in enumerate(world["names"]):
        if "nan" in name or "inf" in name:
            continue
        assert np.array_equal(cs[off[k]:off[k + 1]].view(np.uint32), world["exp_cs"][k].view(np.uint32)), name
    assert np.array_equal(med, world["got"][False][0]) and np.array_equal(med, world["exp"])
