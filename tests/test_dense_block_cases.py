"""The dense random recipe of tests/dense_block_cases.py is well conditioned at every case
tests/test_blocks_dense_gpu.py runs (CPU only), so its 1e-12 cannot quietly rest on an
ill-conditioned input: at each (shape, N, reg_param) the numpy fp64 oracle sits within 1e-14
relative of the long-double recursion (k, K, Hu, pred, lambda, ru, Q, R, M), the smallest Quu
eigenvalue along the DDP recursion is > 0.5, every feasibility flag is true, and the poisoned case
gives exactly [True, False, True].

fxx and fxu are not symmetrised, so the value Hessian is not symmetric and, for nu > 1, neither is
Quu.  noc_ddp_bwd_pass reads Quu as symmetric from its upper triangle (include/noc_hip.h), which
then differs from the reference's full-Quu solve by the asymmetry itself (0.23 relative at
(8, 4), N = 200, against 1e-15 of rounding), so the GPU tests compare with the long-double recursion
under that contract, ddp_bwd_ld(quu="upper").  Both forms are pinned here: the full one against the
oracle, the upper one against its own statements run in fp64, and the eigenvalue bound and the flags
on each."""
import numpy as np
import pytest

import dense_block_cases as C

TOL = 1e-14


def _fp64_upper(Vx, Vxx, derivs, rp):
    """the recursion of ddp_bwd_ld(quu="upper") run in fp64: a correct fp64 ordering of what the
    kernel computes, as the oracle is of the full form"""
    return C.ddp_bwd_ld(Vx, Vxx, derivs, rp, "upper", dtype=np.float64)


def _check_ddp_row(row, rp, want_feasible=True):
    from oracle import noc_oracle as O
    d = C.derivs_of(row)
    for quu, fp64 in (("full", O.ddp_bwd_pass), ("upper", _fp64_upper)):
        info = {}
        k, K, pred, feas, Hu = C.ddp_bwd_ld(row["Vx"], row["Vxx"], d, rp, quu, info)
        assert k.dtype == np.longdouble
        ko, Ko, po, fo, Huo = fp64(row["Vx"], row["Vxx"], d, rp)
        assert feas == fo == want_feasible, quu
        if not want_feasible:
            assert info["min_eig"] < 0
            continue
        for name, a, r in (("k", ko, k), ("K", Ko, K), ("Hu", Huo, Hu), ("pred", po, pred)):
            assert C.rel(a, r) < TOL, (quu, name, C.rel(a, r))
        assert info["min_eig"] > 0.5, (quu, info)


@pytest.mark.parametrize("nx", C.COSTATE_NX)
def test_costate_recipe(nx):
    from oracle import noc_oracle as O
    sizes = [(N, C.COSTATE_B) for N in C.COSTATE_N]
    if nx == C.COSTATE_WIDE[0]:
        sizes.append(C.COSTATE_WIDE[1:])
    for N, B in sizes:
        c = C.costate_case(nx, N, B)
        ref = C.costates_ld(c["lamT"], c["cx"], c["fx"])
        assert ref.dtype == np.longdouble and ref.shape == (B, N + 1, nx)
        for b in range(B):
            lam = O.seq_costates(c["lamT"][b], c["cx"][b], c["fx"][b])
            assert C.rel(lam, ref[b]) < TOL, (N, b, C.rel(lam, ref[b]))
        assert float(np.max(np.abs(ref))) < 50.0, N   # the recursion neither blows up ...
        assert float(np.max(np.abs(ref[:, 0]))) > 1e-2, N   # ... nor dies


@pytest.mark.parametrize("nx,nu", C.LQR_SHAPES)
def test_lqr_params_recipe(nx, nu):
    from oracle import noc_oracle as O
    for N, B in C.LQR_SIZES:
        c, lam = C.lqr_case(nx, nu, N, B)
        names = ("cu", "cxx", "cuu", "cxu", "fu", "fxx", "fuu", "fxu")
        ref = C.lqr_params_ld(lam, *(c[k] for k in names))
        for b in range(B):
            got = O.compute_lqr_params(lam[b], *(c[k][b] for k in names))
            for name, a, r in zip(("ru", "Q", "R", "M"), got, ref):
                assert C.rel(a, r[b]) < TOL, (N, b, name, C.rel(a, r[b]))


@pytest.mark.parametrize("N", C.DDP_N)
@pytest.mark.parametrize("nx,nu", C.DDP_SHAPES)
def test_ddp_recipe(nx, nu, N):
    case, reg = C.ddp_case(nx, nu, N)
    for b in range(3):
        _check_ddp_row(C.row_of(case, b), reg[b])


def test_ddp_recipe_block_boundary_case():
    nx, nu, N, B = C.DDP_WIDE
    case, reg = C.ddp_case(nx, nu, N, B)
    for b in range(B):
        _check_ddp_row(C.row_of(case, b), reg[b])


@pytest.mark.parametrize("nx,nu", C.DDP_BAD)
def test_ddp_recipe_bad_row(nx, nu):
    clean, bad, reg = C.ddp_bad_case(nx, nu)
    for k in clean:   # the poisoned copy differs in cuu[1, 7] only
        same = clean[k] == bad[k]
        if k == "cuu":
            assert not same[1, 7].all()
            same[1, 7] = True
        assert same.all(), k
    for b in range(3):
        _check_ddp_row(C.row_of(bad, b), reg[b], want_feasible=(b != 1))


def test_rows_do_not_depend_on_the_batch_size():
    a, b = C.dense_case(3, 2, 9, 4, 5), C.dense_case(3, 2, 9, 1, 5)
    assert all(np.array_equal(a[k][:1], b[k]) for k in a)
    assert not np.array_equal(a["fx"][0], a["fx"][1])


def test_solve_ld_keeps_extended_precision():
    g = np.random.default_rng(0)
    A = g.normal(size=(4, 4)).astype(np.longdouble) + 4 * np.eye(4)
    Y = g.normal(size=(4, 9)).astype(np.longdouble)
    X = C.solve_ld(A, Y)
    assert X.dtype == np.longdouble
    assert float(np.max(np.abs(A @ X - Y))) < 1e-17   # fp64 would leave ~1e-16
    assert C.solve_ld(A, Y[:, 0]).shape == (4,)
