"""GPU: cm3d_box_vertical through the raw library call against its host statement (cm3d_amd.boxvertical.box_vertical_host) on the lists,
the overflow case and the apply tables of tests/box_vertical_cases.py for every quantile pair -- all five outputs and box TO THE BIT, no
tolerance: a selection has none, and the apply step has no library call and a correctly rounded float64 division on both sides --,
between guard words around every written array; columns 0, 1 and 3 to 9 of box and flags the input's bytes; the overflow case reads
nothing at or beyond idx_cap (those rows are NaN: a read would show as status 4 or as a wrong value); a second call on the arrays the
first one left; every bad-argument call returns its code and launches nothing.  No input provokes a fault: the hostile offsets are
made safe by the clamp the header states."""
import numpy as np
import pytest

from cm3d_amd import boxvertical as bv
from tests import box_vertical_cases as vc

pytestmark = pytest.mark.gpu

CASES = vc.all_cases()
IDS = [c["name"] for c in CASES]
GUARD = 64
I32_GUARD, F64_GUARD = 0x5A5A1234, -7.25e300
ARRAYS = (("vert_z", 2, "d"), ("vert_h", 1, "d"), ("vert_src", 1, "i"), ("vert_status", 1, "i"), ("vert_entry_z", 1, "d"), ("box", vc.BOX_STRIDE, "d"))
PURE = ARRAYS[:5]


def _runs(case):
    """(parameters) of every call of a case: every quantile pair with the case's first run, its other runs with their own parameters."""
    out = [dict(vc.DEFAULTS, q_bot=qb, q_top=qt) for qb, qt in vc.QUANTILES]
    if case["name"] == "apply":
        out = [dict(p, **{k: v for k, v in case["runs"][0].items() if k not in ("q_bot", "q_top")}) for p in out]
    return out + [dict(vc.DEFAULTS, **run) for run in case["runs"]]


@pytest.fixture(scope="module")
def host():
    return {(c["name"], n): bv.box_vertical_host(c["xyz"], c["off"], c["idx_cap"], c["box"], c["flags"], c["prior_wlh"], **p)
            for c in CASES for n, p in enumerate(_runs(c))}


def _guarded(M):
    import torch
    out = {}
    for name, width, kind in ARRAYS:
        dtype, fill = (torch.int32, I32_GUARD) if kind == "i" else (torch.float64, F64_GUARD)
        whole = torch.full((2 * GUARD + M * width,), fill, dtype=dtype, device="cuda")
        out[name] = (whole, whole[GUARD:GUARD + M * width])
    return out


def _guards_intact(bufs):
    for name, width, kind in ARRAYS:
        whole, view = bufs[name]
        w = whole.cpu().numpy()
        fill = I32_GUARD if kind == "i" else F64_GUARD
        n = view.numel()
        assert (w[:GUARD] == fill).all() and (w[GUARD + n:] == fill).all(), name


def _poison(bufs):
    for name, _, kind in PURE:
        bufs[name][1].fill_(12345 if kind == "i" else float("nan"))


def _device_inputs(case):
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return dict(xyz=t(case["xyz"]), off=t(case["off"]), flags=t(case["flags"]), prior_wlh=t(case["prior_wlh"]))


def _raw_call(case, p, bufs, d, fill=True, **override):
    """cm3d_box_vertical through ctypes on the guarded arrays (box filled from the case unless fill is False): the return code.
    override: arguments of the call to replace (a pointer by None)."""
    import torch
    from cm3d_amd import _lib
    L = _lib.lib()
    M = len(case["flags"])
    if fill:
        bufs["box"][1].copy_(torch.from_numpy(case["box"].reshape(-1)).cuda())
    a = dict(p, n_masks=M, idx_cap=case["idx_cap"], n_classes=case["prior_wlh"].shape[0])
    a.update({k: v.data_ptr() for k, v in d.items()})
    a.update({name: bufs[name][1].data_ptr() for name, _, _ in ARRAYS})
    a.update(override)
    rc = L.cm3d_box_vertical(a["xyz"], a["off"], a["n_masks"], a["idx_cap"], a["box"], a["flags"], a["prior_wlh"], a["n_classes"], a["q_bot"],
                             a["q_top"], a["min_points"], a["lo"], a["hi"], a["vert_z"], a["vert_h"], a["vert_src"], a["vert_status"],
                             a["vert_entry_z"], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def _read(bufs, M):
    out = {}
    for name, width, _ in ARRAYS:
        a = bufs[name][1].cpu().numpy()
        out[name] = a.reshape(M, width) if width > 1 else a
    return out


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_device_equals_the_host_statement(case, host):
    M = len(case["flags"])
    bufs, d = _guarded(M), _device_inputs(case)
    others = [c for c in range(vc.BOX_STRIDE) if c != 2]
    for n, p in enumerate(_runs(case)):
        exp = host[case["name"], n]
        _poison(bufs)
        assert _raw_call(case, p, bufs, d) == 0
        got = _read(bufs, M)
        vc.assert_same(got, exp, (case["name"], p))
        assert got["box"][:, others].tobytes() == case["box"][:, others].tobytes()
        assert np.array_equal(d["flags"].cpu().numpy(), case["flags"])
        _guards_intact(bufs)
        if n < 2:
            # a second call on the arrays the first one left: the same box; the entry values are now the first call's
            _poison(bufs)
            assert _raw_call(case, p, bufs, d, fill=False) == 0
            again = _read(bufs, M)
            assert again["box"].tobytes() == got["box"].tobytes() and again["vert_entry_z"].tobytes() == got["box"][:, 2].tobytes()
            for k in ("vert_z", "vert_h", "vert_src", "vert_status"):
                assert again[k].tobytes() == got[k].tobytes(), k
            _guards_intact(bufs)


def test_the_overflow_case_reads_nothing_at_or_beyond_idx_cap():
    """The same call on a copy whose rows from idx_cap on hold other values: the same bytes out.  (And none of them NaN's status.)"""
    from cm3d_amd import ops
    c = vc.overflow_case()
    other = c["xyz"].copy()
    other[c["idx_cap"]:] = 1.0e30
    for kw in c["runs"]:
        p = dict(vc.DEFAULTS, **kw)
        a = ops.box_vertical(c["xyz"], c["off"], c["box"], c["flags"], c["prior_wlh"], idx_cap=c["idx_cap"], **p)
        b = ops.box_vertical(other, c["off"], c["box"], c["flags"], c["prior_wlh"], idx_cap=c["idx_cap"], **p)
        vc.assert_same(a, b, kw)
        assert set(a["vert_status"]) <= {0, 1, 2}
        vc.assert_same(a, bv.box_vertical_host(c["xyz"], c["off"], c["idx_cap"], c["box"], c["flags"], c["prior_wlh"], **p), kw)


def test_empty_batch_and_the_ops_binding():
    from cm3d_amd import ops
    c = vc.apply_case()
    got = ops.box_vertical(c["xyz"], c["off"], c["box"], c["flags"], c["prior_wlh"], **dict(vc.DEFAULTS, **c["runs"][0]))
    vc.assert_same(got, bv.box_vertical_host(c["xyz"], c["off"], c["idx_cap"], c["box"], c["flags"], c["prior_wlh"], **dict(vc.DEFAULTS, **c["runs"][0])))
    none = ops.box_vertical(np.zeros((0, 4), np.float32), [0], np.zeros((0, vc.BOX_STRIDE)), [], c["prior_wlh"])
    assert all(v.shape[0] == 0 for v in none.values())


def test_argument_errors_leave_the_poison():
    """Every bad value and every NULL array: CM3D_ERR_ARG.  Every pure output keeps its poison and box its bytes: nothing was launched."""
    case = vc.apply_case()
    M = len(case["flags"])
    bufs, d = _guarded(M), _device_inputs(case)
    ERR_ARG = -1
    for name, _, _ in PURE:
        bufs[name][1].fill_(42)
    nan, inf = float("nan"), float("inf")
    p = dict(vc.DEFAULTS)
    bad = [dict(q_bot=-0.01), dict(q_top=1.0000001), dict(q_bot=0.6, q_top=0.4), dict(q_bot=nan), dict(q_top=nan), dict(q_bot=nan, q_top=nan),
           dict(min_points=0), dict(min_points=-3), dict(lo=0.0), dict(lo=-1.0), dict(lo=nan), dict(hi=nan), dict(hi=inf), dict(lo=1.3, hi=0.7),
           dict(n_masks=-1), dict(idx_cap=-1), dict(n_classes=-1), dict(n_classes=0)]
    bad += [{k: None} for k in ("xyz", "off", "box", "flags", "prior_wlh", "vert_z", "vert_h", "vert_src", "vert_status", "vert_entry_z")]
    for kw in bad:
        assert _raw_call(case, p, bufs, d, **kw) == ERR_ARG, kw
    for name, _, _ in PURE:
        assert (bufs[name][1].cpu().numpy() == 42).all(), name
    assert _read(bufs, M)["box"].tobytes() == case["box"].tobytes()
    _guards_intact(bufs)
    assert _raw_call(case, p, bufs, d, n_masks=0) == 0                           # no mask: nothing to do, nothing launched
    assert (bufs["vert_src"][1].cpu().numpy() == 42).all()
    assert _raw_call(case, p, bufs, d) == 0                                      # and the same arguments, whole, run
    assert not (bufs["vert_src"][1].cpu().numpy() == 42).any()
    _guards_intact(bufs)
