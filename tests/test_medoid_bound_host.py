"""The error bound behind the medoid's two-pass routes (csrc/medoid.hip: the comment above k_medoid_long, md_inwave_tile),
checked in numpy: with S_j the exact float32 column sums (the reference's chain, correctly rounded roots, ascending sums) and A_j
the sums of roots that are each up to one ulp off,  |A_j - S_j| <= E_j = 1.01 (M + 2) 2^-23 A_j + M 2e-14;  and the tile-local
filter  A_j - E_j <= min_k (A_k + E_k)  over a tile's own columns -- in the float32 form the kernel evaluates, E taken with 1.05
and 2.1e-14 -- keeps the tile's exact first minimum, for tiles of 1 to 64 active columns."""
import numpy as np
import pytest

f32 = np.float32


def _fma32(a, b, c):
    """fmaf on float32 arrays: the product of two float32 is exact in float64; the sum is rounded to odd in float64 (TwoSum tells
    whether anything was lost), so that the final rounding to float32 is the single rounding of the exact value."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = np.broadcast_to(c.astype(np.float64), p.shape)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    fix = (err != 0) & even & np.isfinite(s)
    s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(f32)


def _terms(p):
    """T[i, j]: the reference's float32 distance of row i to column j (torch.cdist's expansion: k-sequential fma chain over
    [-2x_i, -2y_i, -2z_i, n_i, 1] . [x_j, y_j, z_j, 1, n_j], clamp_min_(0), sqrt)."""
    p = p.astype(f32)
    n = ((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]).astype(f32)
    m2 = (f32(-2.0) * p).astype(f32)
    acc = (m2[:, None, 0] * p[None, :, 0]).astype(f32)
    acc = _fma32(np.broadcast_to(m2[:, None, 1], acc.shape), np.broadcast_to(p[None, :, 1], acc.shape), acc)
    acc = _fma32(np.broadcast_to(m2[:, None, 2], acc.shape), np.broadcast_to(p[None, :, 2], acc.shape), acc)
    acc = (acc + n[:, None]).astype(f32)
    acc = (acc + n[None, :]).astype(f32)
    return np.sqrt(np.maximum(acc, f32(0.0))).astype(f32)


def _colsum(T):
    s = np.zeros(T.shape[1], f32)
    for i in range(T.shape[0]):          # ascending rows, float32 adds
        s = (s + T[i]).astype(f32)
    return s


def _ulp_moved(T, how, rng):
    """every root moved by up to one ulp (a root of +0 stays: v_sqrt_f32 of +0 is +0)"""
    up, dn = np.nextafter(T, f32(np.inf)), np.nextafter(T, f32(0.0))
    if how == "up":
        R = up
    elif how == "down":
        R = dn
    else:
        R = np.choose(rng.integers(0, 3, T.shape), [dn, T, up])
    return np.where(T == 0, T, R).astype(f32)


def _lists():
    rng = np.random.default_rng(15)
    out = []
    for name, centre in (("near", (620.0, 1480.0, 1.5)), ("1.7km", (1200.0, 1210.0, 2.0)), ("10km", (7000.0, 7140.0, 2.0)),
                         ("30km", (21000.0, 21400.0, 2.0))):
        for kind, spread in (("random", 40.0), ("object", 2.5), ("clustered", 0.3)):
            for m in (40, 100, 192):
                p = (np.asarray(centre, f32) + rng.uniform(-spread, spread, (m, 3)).astype(f32)).astype(f32)
                out.append((f"{name}_{kind}_{m}", p))
    return out


@pytest.fixture(scope="module")
def sums():
    rng = np.random.default_rng(16)
    out = []
    for name, p in _lists():
        T = _terms(p)
        out.append((name, p, _colsum(T), {how: _colsum(_ulp_moved(T, how, rng)) for how in ("up", "down", "random")}))
    return out


def _E(A, M):
    A = A.astype(np.float64)
    return 1.01 * (M + 2) * 2.0 ** -23 * A + M * 2e-14


def _kernel_filter(A, M):
    """md_inwave_tile's float32 arithmetic: (lower, upper) = (A - E', A + E') with E' = fma(A, 1.05 (M + 2) 2^-23, M 2.1e-14)"""
    rel = (f32(1.05) * f32(M + 2)).astype(f32) * f32(1.1920928955078125e-07)
    e = _fma32(A, np.full_like(A, rel), np.full_like(A, f32(M) * f32(2.1e-14)))
    return (A - e).astype(f32), (A + e).astype(f32), e


def test_the_numpy_chain_is_the_oracle_s(oracle, sums):
    """(the brute force above against orc_medoid's column sums, bit for bit: the fma emulation is exact)"""
    for name, p, S, _ in sums:
        P4 = np.zeros((p.shape[0], 4), f32)
        P4[:, :3] = p
        j, cs = oracle.medoid(P4, np.arange(p.shape[0], dtype=np.int32), want_colsum=True)
        assert np.array_equal(cs.view(np.uint32), S.view(np.uint32)), name
        assert j == int(np.argmin(S)), name


def test_sums_of_one_ulp_roots_stay_inside_the_bound(sums):
    for name, p, S, As in sums:
        M = p.shape[0]
        for how, A in As.items():
            gap = np.abs(A.astype(np.float64) - S.astype(np.float64))
            assert (gap <= _E(A, M)).all(), (name, how, float((gap / _E(A, M)).max()))


def test_the_float32_margin_covers_the_bound(sums):
    """the kernel's float32 E' is never below the E of the derivation, and A -+ E' rounded to float32 still encloses A -+ E"""
    for name, p, S, As in sums:
        M = p.shape[0]
        for how, A in As.items():
            lo, up, e = _kernel_filter(A, M)
            E = _E(A, M)
            assert (e.astype(np.float64) >= E).all(), (name, how)
            assert (lo.astype(np.float64) <= A.astype(np.float64) - E).all() and (up.astype(np.float64) >= A.astype(np.float64) + E).all(), (name, how)


def test_tile_local_candidates_hold_the_exact_first_minimum(sums):
    """A tile = up to 64 consecutive columns of a list; its candidates by the kernel's filter over ITS columns contain the first
    minimum of the exact sums of those columns -- for 1 to 64 active columns, wherever the tile lies in the list."""
    most = 0
    for name, p, S, As in sums:
        M = p.shape[0]
        for how, A in As.items():
            lo, up, _ = _kernel_filter(A, M)
            for nact in range(1, 65):
                for j0 in sorted({0, (M - nact) // 2, M - nact} if nact <= M else ()):
                    sl = slice(j0, j0 + nact)
                    cand = lo[sl] <= up[sl].min()
                    jstar = int(np.argmin(S[sl]))
                    assert cand[jstar], (name, how, nact, j0)
                    assert cand[S[sl] == S[sl][jstar]].all(), (name, how, nact, j0)     # and every exact tie of it
                    most = max(most, int(cand.sum()))
    assert most >= 1
