"""GPU: the first passes of the one-launch DDP kernel (ddp_solve_kernel, csrc/ddp_persistent.hip, behind noc_ddp_solve_ex
and noc_ddp_solve_params) against the high-precision reference of tests/ddp_pass_cases.py.

The kernel carries its own copy of the stage derivatives, the dynamics-Hessian record, the
second-order backward pass, the retry arithmetic, the closed-loop rollout, the lane-chunked cost and
the X/TX, U/TU swap with its copy-out; whole solves (tests/test_ddp.py) see those only through a
fixed point that a wrong term does not move.  With max_passes = k the kernel returns the trial of
pass k whatever was decided about it (D:154), a smooth function of (x0, u0, bp) as long as the
earlier decisions are the reference's, and tests/test_ddp_pass_cases.py holds every one of those
decisions far from its threshold.  So everything numeric is compared at

    bound(k) = max(1e-13, 100 * ORACLE_ERR[k])        (2.5e-11, 6e-12, 5e-12 for k = 1, 2, 3)

in family_cases.own_max_error's measure (max |got - ref| over the field's own maximum): two orders
over the fp64 oracle's own error on the same cases, for the kernel's per-lane-then-wave sums against
the oracle's pairwise ones and generated derivatives against autodiff; counts, flags and
infinities are compared exactly.  Largest device error seen on the MI355X: see DEVICE_ERR below.
"""
import ctypes

import numpy as np
import pytest

import ddp_pass_cases as C
import family_cases as F

pytestmark = pytest.mark.gpu

# largest own-maximum error of any compared field on the MI355X, per pass count (bound above)
# 1: cartpole-N65-bp0.1 gain; 2: the same; 3: pendulum-N63-bp0.1 |Hu| -- the oracle's own error
# on the same fields is 2.0e-13, 4.9e-14, 4.2e-14
DEVICE_ERR = {1: 2.0e-13, 2: 6.5e-14, 3: 4.3e-14}

_TRACE_KEYS = ("bp", "it", "inner", "pred", "gain", "success", "rp", "hu", "cost", "new_cost")


def device_ocp(case):
    from noc import problems
    if case.traced:
        import custom_families as CF
        return CF.cartpole_track_limit(1.0 / case.N)
    if case.name == "linear2":
        return problems.double_integrators(1, F.LINEAR_STEP, constrained=True)
    return problems.make_problem(case.name, case.N)


_SOLVES = {}


def solve(case, k, one_stage=True, trace=False):
    """noc_ddp_solve_ex on the case alone with max_passes = k -> dict(X, U, its, passes, done
    [, trace (k, 10)]); one launch per distinct call and session"""
    key = (case.id, k, one_stage, trace)
    if key not in _SOLVES:
        x0, u0 = C.start(case)
        _SOLVES[key] = run(device_ocp(case), x0[None], u0[None], case.bp, k, one_stage, trace)
    return _SOLVES[key]


def run(ocp, x0, u0, bp, k, one_stage=True, trace=False, params=None):
    import torch
    from noc import _lib
    from noc import differential_dynamic_programming as D
    flags = _lib.DDP_ONE_STAGE if one_stage else 0
    Bt = x0.shape[0]
    if trace:
        lib = _lib.load_for(ocp.family)
        fn = lib.noc_debug_set_ddp_trace
        fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
        buf = torch.zeros(Bt, k, 10, dtype=torch.float64, device="cuda")
        assert fn(buf.data_ptr(), k, Bt) == 0
    try:
        X, U, its, info = D._solve(ocp, u0, x0, "cuda", float(bp), k, flags, params)
        torch.cuda.synchronize()
    finally:
        if trace:
            assert fn(None, 0, 0) == 0
    out = dict(X=X, U=U, its=np.asarray(its), passes=np.asarray(info["passes"]),
               done=np.asarray(info["done"]))
    if trace:
        out["trace"] = buf.cpu().numpy()
    return out


def within(got, ref, k, where):
    """every numeric field of `got` within bound(k) of the reference pass; infinities as such"""
    errs = C.errors(got, ref, tuple(got))
    print("DEVERR", k, where, {f: float(f"{e:.2e}") for f, e in errs.items()})
    for f, e in errs.items():
        assert e <= C.gpu_bound(k), (where, f, e, C.gpu_bound(k))


@pytest.mark.parametrize("case", C.CASES, ids=str)
def test_first_pass_is_decision_free(case):
    """max_passes = 1: the returned controls and states are the reference's first trial -- also
    where that trial leaves the box, as the reference's does -- with and without
    NOC_DDP_ONE_STAGE bit for bit; one iteration, one pass, not done."""
    ref = C.case_passes(case)[0]
    a, b = solve(case, 1, one_stage=True), solve(case, 1, one_stage=False)
    within(dict(TU=a["U"][0], TX=a["X"][0]), ref, 1, case.id)
    for f in ("U", "X", "its", "passes", "done"):
        assert np.array_equal(a[f], b[f]), f
    assert (int(a["its"][0]), int(a["passes"][0]), bool(a["done"][0])) == (1, 1, False)
    if ref["new_cost"] == np.inf:
        assert np.max(np.abs(a["U"])) > float(C.case_row(case)["u_bound"])


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("case", C.CASES, ids=str)
def test_first_k_passes(case, k):
    """max_passes = k: the trial of pass k, and exactly the reference's iteration and pass counts"""
    ref = C.case_passes(case)[k - 1]
    got = solve(case, k)
    within(dict(TU=got["U"][0], TX=got["X"][0]), ref, k, case.id)
    assert (int(got["its"][0]), int(got["passes"][0]), bool(got["done"][0])) == (ref["it"] + 1, k, False)


def _check_trace(rows, refs, bp, where):
    for k, (row, ref) in enumerate(zip(rows, refs), 1):
        t = dict(zip(_TRACE_KEYS, row))
        assert (t["bp"], t["it"], t["inner"], t["success"]) == \
            (bp, ref["it"], ref["inner"], 1.0 if ref["success"] else 0.0), (where, k, t)
        within({f: t[f] for f in C.SCALARS}, ref, k, where)


@pytest.mark.parametrize("case", C.CASES, ids=str)
def test_pass_scalars_through_the_trace(case):
    """The kernel's per-pass diagnostic record (noc_debug_set_ddp_trace): bp, it, inner, success
    exactly; cost, new_cost, pred, gain, rp, |Hu| within the bound, +-inf as such.  A failure of the
    two tests above shows here as cost (cost_feas), pred / |Hu| (backward pass) or new_cost / gain
    (rollout) of the first pass that differs."""
    got = solve(case, C.K, trace=True)
    _check_trace(got["trace"][0], C.case_passes(case), case.bp, case.id)
    plain = solve(case, C.K)
    assert np.array_equal(got["U"], plain["U"]) and np.array_equal(got["X"], plain["X"])


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("name", F.NAMES)
def test_params_rows_follow_their_own_problem(name, k):
    """noc_ddp_solve_params on the heterogeneous twin: row b against the reference run on row b's
    own goal, wx, wu, wf, u_bound (an outside reference for the params kernel's prm.wx read and its
    u_bound, where batch == solo passes a mistake both share)."""
    cases = [c for c in C.TWIN_CASES if c.name == name]
    starts = [C.start(c) for c in cases]
    x0, u0 = np.stack([s[0] for s in starts]), np.stack([s[1] for s in starts])
    got = run(device_ocp(cases[0]), x0, u0, C.TWIN_BP, k, params=C.twin_params(name))
    for b, c in enumerate(cases):
        ref = C.case_passes(c)[k - 1]
        within(dict(TU=got["U"][b], TX=got["X"][b]), ref, k, c.id)
        assert (int(got["its"][b]), int(got["passes"][b]), bool(got["done"][b])) == \
            (ref["it"] + 1, k, False), c.id


@pytest.mark.parametrize("name", F.NAMES)
def test_batch_rows_equal_solo_at_the_cap(name):
    """three different starts of one family and horizon (N = 65) in one launch, max_passes = 2:
    every row bit-equal to its solo solve -- controls, states, iterations, passes, done"""
    case = C.BY_ID[f"{name}-N65-bp0.1"]
    starts = [C.start(case, rep) for rep in range(3)]
    x0, u0 = np.stack([s[0] for s in starts]), np.stack([s[1] for s in starts])
    ocp = device_ocp(case)
    batch = run(ocp, x0, u0, case.bp, 2)
    assert len({batch["U"][b].tobytes() for b in range(3)}) == 3
    for b in range(3):
        solo = run(ocp, x0[b:b + 1], u0[b:b + 1], case.bp, 2)
        for f in ("U", "X", "its", "passes", "done"):
            assert np.array_equal(batch[f][b], solo[f][0]), (b, f)


@pytest.mark.parametrize("k", [1, 2, 3])
def test_traced_cost_family_first_passes(k):
    """The kGenCost path of the record (CXX, CUU, CXU from stage_hess): the traced-cost cart-pole
    of tests/custom_families.py (quartic pole-rate penalty, track limit inside the log barrier),
    started away from rest, against the same reference (its cost is restated in mpmath,
    ddp_pass_cases.TracedCartpole) at the same bound; k = 3 also through the trace."""
    case = C.TRACED_CASE
    ref = C.case_passes(case)
    got = solve(case, k, trace=(k == C.K))
    within(dict(TU=got["U"][0], TX=got["X"][0]), ref[k - 1], k, case.id)
    assert (int(got["its"][0]), int(got["passes"][0]), bool(got["done"][0])) == \
        (ref[k - 1]["it"] + 1, k, False)
    if k == C.K:
        _check_trace(got["trace"][0], ref, case.bp, case.id)
