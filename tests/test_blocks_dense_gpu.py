"""The stand-alone building-block kernels (csrc/derivatives.hip, csrc/ddp_blocks.hip) at the shapes
where their loops actually run, against plain long-double recursions (tests/dense_block_cases.py).

noc_costates, noc_lqr_params and noc_ddp_bwd_pass take raw arrays, so they are driven with dense
random data (no structural zero, fxx / fxu / cxu unsymmetrised) at every supported shape:
  * costates: nx = 1..8, N up to 200 -- lane chunks of length 2, 3 and 4 in the parallel scan's
    in-chunk sweep, rem != 0 with base >= 1, more than one compose step; B = 65 for the sequential
    kernel's second block;
  * LQ parameters: nu > 1 (and nu > nx), 259 threads, so a block boundary inside a trajectory;
  * DDP backward pass: (8, 4) with non-zero fxx, fxu, fuu, cxu; B = 66; an indefinite Quu in one row.
The family-bound kernels get the remaining block-boundary and stride cases: total_cost at N > 64,
compute_derivatives at 296 threads, final_cost_grad at B = 257, nonlin_rollout at B = 65.

Tolerance: 1e-12 relative (max|a - r| / max(1, max|r|)) wherever a long-double reference is
compared.  Two correct fp64 orderings of these recursions sit <= 1e-15 from it on this recipe
(tests/test_dense_block_cases.py asserts 1e-14 on the CPU at every case used here); 1e-12 leaves
three orders for FMA contraction and the scan's association and is far below any indexing error.
The family-bound cases keep the tolerances of the tests they extend (total_cost and nonlin_rollout
1e-12, derivatives against autodiff 1e-10).

noc_ddp_bwd_pass reads Quu as symmetric from its upper triangle (include/noc_hip.h).  With fxx
unsymmetrised the value Hessian is not symmetric, so for nu > 1 neither is Quu, and the reference's
full-Quu solve (D:50-55) is a different number: 0.23 relative at (8, 4), N = 200 in long double.
The reference here is therefore the long-double recursion with Quu mirrored from its upper triangle
(ddp_bwd_ld(quu="upper")): the statements of D:28-70 under the entry point's stated contract.  A
transposed index in fxx, fxu or cxu still shows: in the long-double model, swapping two axes of fxx
or fxu at (8, 4), N = 65 moves k, K, Hu, pred by 0.2 relative.

"Guarded" outputs are slices of NaN-filled buffers with 64 guard elements on each side: no NaN may
remain inside (a stage a thread forgot) and both guards must be untouched.  Every direct call of
noc_lqr_params and noc_ddp_bwd_pass here is guarded; the costates go through noc.costates.costates
except at nx = 5, N = 2 / 65 / 130, where the direct call is guarded.

Largest relative error observed on an MI355X (gfx950), per kernel, over all cases of this file:
  costates_par_kernel    7.5e-16  (nx = 8, N = 64)
  costates_seq_kernel    5.5e-16  (nx = 8, N = 200)
  lqr_params_kernel      5.1e-16  ((8, 4), N = 37, Q)
  ddp_bwd_kernel         1.5e-15  ((8, 4), N = 200, reg_param 1e-3, pred)
  total_cost_kernel      5.6e-16  (pendulum, N = 64; against the host callable)
  nonlin_rollout_kernel  1.1e-16  (nx = 8 stack; against the oracle's rollout)
  derivatives_kernel     2.2e-16  (cart-pole fx; against autodiff, bound 1e-10)
No kernel needs more than 1e-12, and none was found wrong.
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import dense_block_cases as C

pytestmark = pytest.mark.gpu

TOL = 1e-12
GUARD = 64


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")


def _report(kernel, what, err):
    """every figure is printed before it is asserted (pytest -s shows them)"""
    print(f"observed {kernel} {what} {err:.3e}")
    return err


class _Guarded:
    """an output of `shape` inside a larger buffer: fp64 buffers are NaN-filled, int32 ones hold a
    sentinel, GUARD elements on each side"""

    def __init__(self, shape, dtype=torch.float64):
        n = int(np.prod(shape))
        self.fill = float("nan") if dtype == torch.float64 else -7
        self.buf = torch.full((n + 2 * GUARD,), self.fill, dtype=dtype, device="cuda")
        self.bits = self.buf.view(torch.int64 if dtype == torch.float64 else torch.int32)
        self.before = self.bits.clone()
        self.view = self.buf[GUARD:GUARD + n].view(*shape)

    def data_ptr(self):
        return self.view.data_ptr()

    def check(self, name):
        lo, hi = slice(0, GUARD), slice(self.buf.numel() - GUARD, self.buf.numel())
        assert torch.equal(self.bits[lo], self.before[lo]), f"{name}: guard before the output written"
        assert torch.equal(self.bits[hi], self.before[hi]), f"{name}: guard after the output written"
        if self.buf.dtype == torch.float64:
            assert not bool(torch.isnan(self.view).any()), f"{name}: an element was never written"
        else:
            assert bool(((self.view == 0) | (self.view == 1)).all()), f"{name}: never written"
        return self.view.cpu().numpy()


# ------------------------------------------------------------------------------------- costates
@functools.lru_cache(maxsize=None)
def _costate_ref(nx, N, B):
    c = C.costate_case(nx, N, B)
    return c, C.costates_ld(c["lamT"], c["cx"], c["fx"]).astype(np.float64)


def _costates(c, sequential, rows=slice(None)):
    from noc.costates import costates
    lam = costates(c["lamT"][rows], c["cx"][rows], c["fx"][rows], sequential=sequential)
    torch.cuda.synchronize()
    return lam.cpu().numpy()


def _costates_guarded(c, sequential):
    from noc import _lib
    B, N, nx = c["cx"].shape
    lamT, cx, fx = _dev(c["lamT"]), _dev(c["cx"]), _dev(c["fx"])
    out = _Guarded((B, N + 1, nx))
    lib = _lib.load()
    _lib.check(lib.noc_costates(nx, N, B, lamT.data_ptr(), cx.data_ptr(), fx.data_ptr(),
                                out.data_ptr(), 1 if sequential else 0,
                                _lib.stream_handle(cx.device)), "noc_costates", lib)
    torch.cuda.synchronize()
    return out.check("lam")


@pytest.mark.parametrize("sequential", [False, True], ids=["par", "seq"])
@pytest.mark.parametrize("N", C.COSTATE_N)
@pytest.mark.parametrize("nx", C.COSTATE_NX)
def test_costates_dense(nx, N, sequential):
    """N = 63: every lane but the last one stage; 64: one each; 65: lane 0 two (rem = 1, base = 1);
    130: 3 / 2; 200: 4 / 3 -- the in-chunk sweep and the compose loop run up to three / four times"""
    c, ref = _costate_ref(nx, N, C.COSTATE_B)
    lam = _costates(c, sequential)
    kernel = "costates_seq_kernel" if sequential else "costates_par_kernel"
    assert _report(kernel, f"nx={nx} N={N}", C.rel(lam, ref)) < TOL


@pytest.mark.parametrize("sequential", [False, True], ids=["par", "seq"])
@pytest.mark.parametrize("N", [2, 65, 130])
def test_costates_guarded(N, sequential):
    c, ref = _costate_ref(5, N, C.COSTATE_B)
    lam = _costates_guarded(c, sequential)
    assert C.rel(lam, ref) < TOL
    assert np.array_equal(lam, _costates(c, sequential))   # the wrapper makes the same call


@pytest.mark.parametrize("sequential", [False, True], ids=["par", "seq"])
def test_costates_second_block(sequential):
    """B = 65: trajectory 64 is thread 0 of the sequential kernel's block 1 (63 idle threads behind
    it); rows are bit for bit what the same row gives alone"""
    nx, N, B = C.COSTATE_WIDE
    c, ref = _costate_ref(nx, N, B)
    lam = _costates(c, sequential)
    kernel = "costates_seq_kernel" if sequential else "costates_par_kernel"
    for b in range(B):
        assert _report(kernel, f"B=65 row {b}", C.rel(lam[b], ref[b])) < TOL, b
    for b in (0, 63, 64):
        assert np.array_equal(lam[b], _costates(c, sequential, slice(b, b + 1))[0]), b


# -------------------------------------------------------------------------------- LQ parameters
_LQR_IN = ("cu", "cxx", "cuu", "cxu", "fu", "fxx", "fuu", "fxu")


def _lqr_params(c, lam):
    from noc import _lib
    B, N, nx = c["cx"].shape
    nu = c["cu"].shape[-1]
    ins = [_dev(lam)] + [_dev(c[k]) for k in _LQR_IN]
    outs = dict(ru=_Guarded((B, N, nu)), Q=_Guarded((B, N, nx, nx)), R=_Guarded((B, N, nu, nu)),
                M=_Guarded((B, N, nx, nu)))
    lib = _lib.load()
    _lib.check(lib.noc_lqr_params(nx, nu, N, B, *(t.data_ptr() for t in ins),
                                  *(outs[k].data_ptr() for k in ("ru", "Q", "R", "M")),
                                  _lib.stream_handle(ins[0].device)), "noc_lqr_params", lib)
    torch.cuda.synchronize()
    return {k: v.check(k) for k, v in outs.items()}


@pytest.mark.parametrize("N,B", C.LQR_SIZES)
@pytest.mark.parametrize("nx,nu", C.LQR_SHAPES)
def test_lqr_params_dense(nx, nu, N, B):
    """nu > 1 separates (bk*nx+i)*nu+j from its transposes and the fuu / fxu strides from each
    other; (5, 8) has nu > nx; N = 37, B = 7 is 259 threads: block 1 starts at stage 34 of
    trajectory 6.  Every output guarded (the issue asks for (3, 2) and (8, 4); all are)."""
    c, lam = C.lqr_case(nx, nu, N, B)
    got = _lqr_params(c, lam)
    ref = C.lqr_params_ld(lam, *(c[k] for k in _LQR_IN))
    for name, r in zip(("ru", "Q", "R", "M"), ref):
        err = _report("lqr_params_kernel", f"({nx},{nu}) N={N} {name}", C.rel(got[name], r))
        assert err < TOL, name


# ---------------------------------------------------------------------------- DDP backward pass
def _ddp_bwd(c, reg, rows=slice(None)):
    """noc_ddp_bwd_pass on rows `rows` of a case -> dict of numpy k, K, pred, feasible, Hu
    (every output guarded)"""
    from noc import _lib
    cx = c["cx"][rows]
    B, N, nx = cx.shape
    nu = c["cu"].shape[-1]
    ins = [_dev(c["Vx"][rows]), _dev(c["Vxx"][rows]), _dev(np.asarray(reg, np.float64)[rows])]
    ins += [_dev(c[k][rows]) for k in C.FIELDS]
    outs = dict(k=_Guarded((B, N, nu)), K=_Guarded((B, N, nu, nx)), pred=_Guarded((B,)),
                feasible=_Guarded((B,), torch.int32), Hu=_Guarded((B, N, nu)))
    lib = _lib.for_shape(nx, nu)
    _lib.check(lib.noc_ddp_bwd_pass(nx, nu, N, B, *(t.data_ptr() for t in ins),
                                    *(outs[k].data_ptr() for k in ("k", "K", "pred", "feasible", "Hu")),
                                    _lib.stream_handle(ins[0].device)), "noc_ddp_bwd_pass", lib)
    torch.cuda.synchronize()
    return {k: v.check(k) for k, v in outs.items()}


def _ddp_ref_row(c, reg, b):
    row = C.row_of(c, b)
    k, K, pred, feas, Hu = C.ddp_bwd_ld(row["Vx"], row["Vxx"], C.derivs_of(row), reg[b], quu="upper")
    assert feas
    return dict(k=k.astype(np.float64), K=K.astype(np.float64), pred=float(pred),
                Hu=Hu.astype(np.float64))


def _assert_ddp_row(got, ref, b, what):
    for name in ("k", "K", "Hu", "pred"):
        err = _report("ddp_bwd_kernel", f"{what} row {b} {name}", C.rel(got[name][b], ref[name]))
        assert err < TOL, (b, name)


def _rows_bit_identical(full, solo, b):
    return all(np.array_equal(full[k][b], solo[k][0]) for k in full)


@pytest.mark.parametrize("N", C.DDP_N)
@pytest.mark.parametrize("nx,nu", C.DDP_SHAPES)
def test_ddp_bwd_pass_dense(nx, nu, N):
    """every contraction of the backward pass multiplied by non-zero numbers: Vx . fxx / fxu / fuu,
    cxu, ldl_solve<NU, NX + 1>; reg_param 0, 1e-3 and 25 in rows 0, 1, 2"""
    c, reg = C.ddp_case(nx, nu, N)
    got = _ddp_bwd(c, reg)
    assert got["feasible"].tolist() == [1, 1, 1]
    for b in range(3):
        _assert_ddp_row(got, _ddp_ref_row(c, reg, b), b, f"({nx},{nu}) N={N}")


def test_ddp_bwd_pass_second_block():
    """B = 66 in 64-thread blocks: rows 64 and 65 are block 1, 62 threads past the batch"""
    nx, nu, N, B = C.DDP_WIDE
    c, reg = C.ddp_case(nx, nu, N, B)
    got = _ddp_bwd(c, reg)
    assert got["feasible"].tolist() == [1] * B
    for b in range(B):
        _assert_ddp_row(got, _ddp_ref_row(c, reg, b), b, "B=66")
    for b in (0, 63, 64, 65):
        assert _rows_bit_identical(got, _ddp_bwd(c, reg, slice(b, b + 1)), b), b


@pytest.mark.parametrize("nx,nu", C.DDP_BAD)
def test_ddp_bwd_pass_bad_row(nx, nu):
    """row 1 has cuu[7] = -5 I: its flag is 0, and its neighbours in the block do not notice (row
    1's numbers are not compared: LDL' without pivoting on an indefinite Quu need not match LU)"""
    clean, bad, reg = C.ddp_bad_case(nx, nu)
    good, got = _ddp_bwd(clean, reg), _ddp_bwd(bad, reg)
    assert good["feasible"].tolist() == [1, 1, 1] and got["feasible"].tolist() == [1, 0, 1]
    for b in (0, 2):
        assert all(np.array_equal(got[k][b], good[k][b]) for k in got), b
        _assert_ddp_row(got, _ddp_ref_row(bad, reg, b), b, f"bad ({nx},{nu})")


# ------------------------------------------------------------------------ family-bound kernels
def _rolled(ocp, x0, u0):
    from noc.utils import rollout
    return np.stack([rollout(ocp.dynamics, u0[b], x0[b]) for b in range(len(u0))])


@pytest.mark.parametrize("N", [64, 65, 130])
@pytest.mark.parametrize("name", ["pendulum", "cartpole", "linear8"])
def test_total_cost_strides_past_one_wave(name, N):
    """the lanes stride the stages by 64: N = 64 is one full trip, 65 a second trip of lane 0
    alone, 130 three.  Against the OCP's host total_cost at 1e-12 (as
    test_ddp.py::test_total_cost_matches_the_ocp_callable), per-trajectory bp."""
    from noc.par_interior_point_newton import total_cost
    from test_ddp_params_gpu import _case
    ocp, x0, u0, params, solo = _case(name, N, 3)
    X = _rolled(ocp, x0, u0)
    bp = np.array([0.1, 0.02, 1e-3])
    got = total_cost(ocp, X, u0, torch.tensor(bp, device="cuda")).cpu().numpy()
    for b in range(3):
        want = ocp.total_cost(X[b], u0[b], bp[b])
        err = abs(got[b] - want) / max(1.0, abs(want))
        assert _report("total_cost_kernel", f"{name} N={N} row {b}", err) <= 1e-12, (b, got[b], want)
    if N == 130:
        bad = u0.copy()
        bad[1, 100, 0] = 2 * ocp.family.u_bound   # the second trip of lane 36
        nan = total_cost(ocp, X, bad, torch.tensor(bp, device="cuda")).cpu().numpy()
        assert np.isnan(nan[1]) and nan[0] == got[0] and nan[2] == got[2]
        with_params = total_cost(ocp, X, u0, torch.tensor(bp, device="cuda"), params=params)
        assert bool(torch.isfinite(with_params).all())
        for b in range(3):
            sl = slice(b, b + 1)
            one = total_cost(solo[b], X[sl], u0[sl], torch.tensor(bp[sl], device="cuda"))
            assert torch.equal(with_params[b], one[0]), b
        assert len({float(v) for v in with_params}) == 3   # the rows are different problems


@pytest.mark.parametrize("name", ["pendulum", "cartpole"])
def test_compute_derivatives_second_block(name):
    """N = 37, B = 8 is 296 (trajectory, stage) threads: block 1 starts at stage 34 of trajectory
    6, so rows 6 and 7 are checked against the oracle's autodiff (1e-10, as test_api_gpu.py);
    every row is bit for bit its own B = 1 call, also with per-trajectory parameters (the record
    pick tt / N)."""
    from noc.par_interior_point_newton import compute_derivatives
    from test_api_gpu import _case, _rel
    from test_ddp_params_gpu import _rows
    N, B = 37, 8
    ocp, prob, x0, u0, X = _case(name, N, B, 3)
    bp = np.array([0.1, 0.02, 0.004, 0.1, 0.02, 0.004, 0.1, 0.02])
    d = compute_derivatives(ocp, X, u0, bp)
    for b in (6, 7):
        ref = prob.derivatives(X[b], u0[b], bp[b])
        for k, r in zip(d._fields, ref):
            err = _rel(getattr(d, k)[b].cpu(), r)
            assert _report("derivatives_kernel", f"{name} row {b} {k}", err) < 1e-10, (b, k)
    params, solo = _rows(ocp.family, B)
    dp = compute_derivatives(ocp, X, u0, bp, params=params)
    for b in range(B):
        sl = slice(b, b + 1)
        d1 = compute_derivatives(ocp, X[sl], u0[sl], bp[sl])
        ds = compute_derivatives(ocp._replace(family=solo[b]), X[sl], u0[sl], bp[sl])
        for k in d._fields:
            assert torch.equal(getattr(d, k)[b], getattr(d1, k)[0]), (b, k)
            assert torch.equal(getattr(dp, k)[b], getattr(ds, k)[0]), (b, k)
    assert not torch.equal(dp.cx, d.cx) and not torch.equal(dp.cuu, d.cuu)


def test_final_cost_grad_second_block():
    """B = 257 in 256-thread blocks: trajectory 256 is thread 0 of block 1 (final_derivs_kernel
    and its per-trajectory-parameter twin)"""
    from noc import problems
    from noc.costates import final_cost_grad
    B = 257
    ocp = problems.make_problem("cartpole", 30)
    xN = np.random.default_rng(21).normal(size=(B, 4))
    g, H = final_cost_grad(ocp, xN, hessian=True)
    assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(H).all())
    for b in (0, 255, 256):
        g1, H1 = final_cost_grad(ocp, xN[b:b + 1], hessian=True)
        assert torch.equal(g[b], g1[0]) and torch.equal(H[b], H1[0]), b
    assert not torch.equal(g[255], g[256])
    # final_derivs_kernel with records: the same boundary with one record per trajectory
    from test_ddp_params_gpu import _rows
    params, solo = _rows(ocp.family, B)
    gp, Hp = final_cost_grad(ocp, xN, hessian=True, params=params)
    for b in (0, 255, 256):
        g1, H1 = final_cost_grad(ocp._replace(family=solo[b]), xN[b:b + 1], hessian=True)
        assert torch.equal(gp[b], g1[0]) and torch.equal(Hp[b], H1[0]), b
    assert not torch.equal(gp, g)


@pytest.mark.parametrize("name,N", [("pendulum", 70), ("linear8", 20)])
def test_nonlin_rollout_second_block(name, N):
    """B = 65 in 64-thread blocks; rows 0, 63, 64 against the oracle's rollout at 1e-12 (as
    test_ddp.py::test_ddp_bwd_pass_and_nonlin_rollout_match_oracle)"""
    from noc.par_interior_point_newton import nonlin_rollout
    from oracle import noc_oracle as O, problems as PR
    from test_ddp import _oracle_problem
    from test_ddp_params_gpu import _case
    B = 65
    ocp, x0, u0, _, _ = _case(name, N, B)
    prob = (_oracle_problem(name, N) if name == "pendulum"
            else O.NumpyProblem(PR.linear_ocp(4, 0.1, constrained=True)))
    X = _rolled(ocp, x0, u0)
    rng = np.random.default_rng(31)
    nx, nu = ocp.family.nx, ocp.family.nu
    K, k = 0.05 * rng.normal(size=(B, N, nu, nx)), 0.01 * rng.normal(size=(B, N, nu))
    TX, TU = (t.cpu().numpy() for t in nonlin_rollout(ocp, K, k, X, u0))
    assert np.isfinite(TX).all() and np.isfinite(TU).all()
    for b in (0, 63, 64):
        TXr, TUr = O.ddp_nonlin_rollout(prob, K[b], k[b], X[b], u0[b])
        ex, eu = C.rel(TX[b], TXr), C.rel(TU[b], TUr)
        _report("nonlin_rollout_kernel", f"{name} row {b}", max(ex, eu))
        assert ex < 1e-12 and eu < 1e-12, b
    assert not np.array_equal(TX[63], TX[64])
