"""Dense random inputs and extended-precision references for the raw-array building blocks
(noc_costates, noc_lqr_params, noc_ddp_bwd_pass).  A helper, not a test: it never touches the GPU.

`dense_case(nx, nu, N, B, seed)` draws every Derivatives array and the terminal values with no
structural zero and no accidental symmetry, so that an index expression of a kernel cannot be told
from a wrong one only where the mathematics cannot either:

    fx    0.95 * Q_k + 0.02 * randn    Q_k the orthogonal factor of a QR of randn(nx, nx): the costate
                                       and value recursions neither blow up nor die over N = 200
    fu    0.3 * randn
    cx, cu  randn
    cxx   I + 0.1 * sym(randn)
    cuu   I + 0.1 * sym(randn)         symmetric: noc_ddp_bwd_pass reads Quu's upper triangle
    cxu   0.1 * randn
    fxx   0.01 * randn                 NOT symmetrised: a transposed (i, j) shows
    fxu   0.01 * randn                 NOT symmetrised
    fuu   0.01 * randn                 symmetrised over its last two axes (as cuu)
    Vx = lamT  randn
    Vxx   I + 0.1 * sym(randn)

The second derivatives' scale is 0.01, not a larger one: with fxx unsymmetrised the value Hessian
picks up an antisymmetric part, and at 0.02 the reference's full-Quu recursion (reg_param 0, shape
(8, 4), N >= 65) amplifies it until Quu turns indefinite and |Vxx| reaches 1e42.  At 0.01 both forms
of the recursion stay bounded (|Vxx| <= 14, |Vx| <= 12, smallest Quu eigenvalue >= 0.68 over four
seeds); tests/test_dense_block_cases.py holds that on the cases used.

Row b of a case depends on (nx, nu, N, seed, b) only, not on B: a row of a large batch is the same
data as that row drawn alone.

The references run the plain recursions in np.longdouble (64-bit mantissa on x86-64): costates_ld
(C:43-54), lqr_params_ld (P:31-42, the einsums of oracle.noc_oracle.compute_lqr_params) and
ddp_bwd_ld (D:28-70, statement for statement as oracle.noc_oracle.ddp_bwd_pass, with a pivoted
elimination written out because np.linalg.solve would drop to fp64).  They return long double;
callers cast to fp64 to compare.

ddp_bwd_ld(..., quu="upper") is the recursion under the contract include/noc_hip.h states for
noc_ddp_bwd_pass: Quu is READ AS SYMMETRIC from its upper triangle.  With fxx unsymmetrised, Qxx
and so Vxx are not symmetric after the first stage, fu' Vxx fu is then not symmetric for nu > 1, and
the reference's solve with the full Quu (quu="full", D:50-55) and the kernel's solve with the
mirrored upper triangle are different numbers -- by the asymmetry, not by rounding.  The GPU tests
compare with quu="upper"; the CPU recipe test pins both forms.
"""
import numpy as np

LD = np.longdouble
SECOND = 0.01   # scale of the dynamics' second derivatives fxx, fxu, fuu (see the module docstring)
FIELDS = ("cx", "cu", "cxx", "cuu", "cxu", "fx", "fu", "fxx", "fuu", "fxu")  # Derivatives order


def rel(a, r):
    """max|a - r| / max(1, max|r|), the measure of tests/test_api_gpu.py"""
    a, r = np.asarray(a, np.float64), np.asarray(r, np.float64)
    return float(np.max(np.abs(a - r)) / max(1.0, float(np.max(np.abs(r)))))


def _sym(a):
    return 0.5 * (a + np.swapaxes(a, -1, -2))


def _row(nx, nu, N, seed, b):
    g = np.random.default_rng([int(seed), int(b), nx, nu, N])
    q, _ = np.linalg.qr(g.normal(size=(N, nx, nx)))
    return dict(
        fx=0.95 * q + 0.02 * g.normal(size=(N, nx, nx)),
        fu=0.3 * g.normal(size=(N, nx, nu)),
        cx=g.normal(size=(N, nx)),
        cu=g.normal(size=(N, nu)),
        cxx=np.eye(nx) + 0.1 * _sym(g.normal(size=(N, nx, nx))),
        cuu=np.eye(nu) + 0.1 * _sym(g.normal(size=(N, nu, nu))),
        cxu=0.1 * g.normal(size=(N, nx, nu)),
        fxx=SECOND * g.normal(size=(N, nx, nx, nx)),
        fxu=SECOND * g.normal(size=(N, nx, nx, nu)),
        fuu=SECOND * _sym(g.normal(size=(N, nx, nu, nu))),
        Vx=g.normal(size=(nx,)),
        Vxx=np.eye(nx) + 0.1 * _sym(g.normal(size=(nx, nx))),
    )


def dense_case(nx, nu, N, B, seed):
    """dict of C-contiguous fp64 arrays with a leading batch axis B, in the ABI's natural layout:
    the ten Derivatives FIELDS, Vx (B, nx) (also under the name lamT) and Vxx (B, nx, nx)."""
    rows = [_row(nx, nu, N, seed, b) for b in range(B)]
    c = {k: np.ascontiguousarray(np.stack([r[k] for r in rows])) for k in rows[0]}
    c["lamT"] = c["Vx"]
    return c


def row_of(case, b):
    """trajectory b of a case, without the batch axis"""
    return {k: v[b] for k, v in case.items()}


def derivs_of(row):
    """the Derivatives tuple of one trajectory, in the oracle's order"""
    return tuple(row[k] for k in FIELDS)


# ------------------------------------------------------------------------------------------------
def costates_ld(lamT, cx, fx):
    """lambda_N = lamT, lambda_k = cx_k + fx_k' lambda_{k+1}; batched (B, ...) -> (B, N+1, nx)"""
    lamT, cx, fx = (np.asarray(a, LD) for a in (lamT, cx, fx))
    B, N, nx = cx.shape
    lam = np.zeros((B, N + 1, nx), LD)
    lam[:, N] = lamT
    for k in range(N - 1, -1, -1):
        lam[:, k] = cx[:, k] + np.einsum("bmi,bm->bi", fx[:, k], lam[:, k + 1])
    return lam


def lqr_params_ld(lam, cu, cxx, cuu, cxu, fu, fxx, fuu, fxu):
    """ru, Q, R, M with l = lambda[:, 1:]; batched (B, ...)"""
    lam, cu, cxx, cuu, cxu, fu, fxx, fuu, fxu = (np.asarray(a, LD) for a in
                                                 (lam, cu, cxx, cuu, cxu, fu, fxx, fuu, fxu))
    l = lam[:, 1:]
    ru = cu + np.einsum("bkij,bki->bkj", fu, l)
    Q = cxx + np.einsum("bki,bkijl->bkjl", l, fxx)
    R = cuu + np.einsum("bki,bkijl->bkjl", l, fuu)
    M = cxu + np.einsum("bki,bkijl->bkjl", l, fxu)
    return ru, Q, R, M


def solve_ld(A, Y, dtype=LD):
    """A^-1 Y by Gaussian elimination with partial pivoting, in long double"""
    A, Y = np.array(A, dtype), np.array(Y, dtype)
    vec = Y.ndim == 1
    if vec:
        Y = Y[:, None]
    n = A.shape[0]
    for j in range(n):
        p = j + int(np.argmax(np.abs(A[j:, j])))
        if p != j:
            A[[j, p]], Y[[j, p]] = A[[p, j]], Y[[p, j]]
        for i in range(j + 1, n):
            f = A[i, j] / A[j, j]
            A[i, j:] -= f * A[j, j:]
            Y[i] -= f * Y[j]
    X = np.zeros_like(Y)
    for i in range(n - 1, -1, -1):
        X[i] = (Y[i] - A[i, i + 1:] @ X[i + 1:]) / A[i, i]
    return X[:, 0] if vec else X


def ddp_bwd_ld(Vx_T, Vxx_T, derivs, reg_param, quu="full", info=None, dtype=LD):
    """D:28-70 for one trajectory in long double -> (k, K, pred, feasible, Hu).
    quu="full": the reference's statements; quu="upper": Quu mirrored from its upper triangle before
    the eigenvalue test and the solves (the contract of noc_ddp_bwd_pass).  info (a dict) receives
    min_eig, the smallest eigenvalue of any stage's Quu as solved (fp64 eigvalsh of the cast), and
    max_Vxx, max_Vx, max_Quu, the largest magnitudes along the recursion.  dtype=np.float64 runs
    the very same statements in fp64 (the recipe test measures the recursion's conditioning with
    it)."""
    LD = dtype
    cx, cu, cxx, cuu, cxu, fx, fu, fxx, fuu, fxu = (np.asarray(a, LD) for a in derivs)
    N, nu = cu.shape
    nx = cx.shape[1]
    reg = LD(reg_param) * np.sqrt(np.sum(cu * cu))                       # D:34-35
    Vx, Vxx = np.asarray(Vx_T, LD), np.asarray(Vxx_T, LD)
    k, K, Hu = np.zeros((N, nu), LD), np.zeros((N, nu, nx), LD), np.zeros((N, nu), LD)
    dV = np.zeros(N, LD)
    feasible, min_eig, max_Vxx, max_Vx, max_Quu = True, np.inf, 0.0, 0.0, 0.0
    for t in range(N - 1, -1, -1):
        Qx = cx[t] + fx[t].T @ Vx                                        # D:41
        Qu = cu[t] + fu[t].T @ Vx                                        # D:42
        Qxx = cxx[t] + fx[t].T @ Vxx @ fx[t] + np.tensordot(Vx, fxx[t], axes=1)   # D:43
        Qxu = cxu[t] + fx[t].T @ Vxx @ fu[t] + np.tensordot(Vx, fxu[t], axes=1)   # D:44
        Quu = cuu[t] + fu[t].T @ Vxx @ fu[t] + np.tensordot(Vx, fuu[t], axes=1)   # D:45
        Quu = Quu + reg * np.eye(nu, dtype=LD)                           # D:46
        if quu == "upper":
            Quu = np.triu(Quu) + np.triu(Quu, 1).T
        elif quu != "full":
            raise ValueError(quu)
        ev = float(np.min(np.linalg.eigvalsh(_sym(Quu.astype(np.float64)))))
        min_eig = min(min_eig, ev)
        max_Quu = max(max_Quu, float(np.max(np.abs(Quu))))
        feasible &= ev > 0                                            # D:47-48
        sol = solve_ld(Quu, np.concatenate([Qu[:, None], Qxu.T], axis=1), LD)
        iQu, iQxuT = sol[:, 0], sol[:, 1:]
        k[t] = -iQu                                                      # D:50
        K[t] = -iQxuT                                                    # D:51
        dV[t] = -0.5 * Qu @ iQu                                          # D:53
        Vx = Qx - Qu @ iQxuT                                             # D:54
        Vxx = Qxx - Qxu @ iQxuT                                          # D:55
        Hu[t] = Qu
        max_Vxx = max(max_Vxx, float(np.max(np.abs(Vxx))))
        max_Vx = max(max_Vx, float(np.max(np.abs(Vx))))
    if info is not None:
        info.update(min_eig=min_eig, max_Vxx=max_Vxx, max_Vx=max_Vx, max_Quu=max_Quu)
    return k, K, dV.sum(), feasible, Hu                                  # D:61-70


def poison_row(case, b=1, stage=7):
    """a copy of `case` whose trajectory b has cuu[stage] = -5 I: Quu there is indefinite"""
    bad = {k: v.copy() for k, v in case.items()}
    bad["lamT"] = bad["Vx"]
    nu = bad["cuu"].shape[-1]
    bad["cuu"][b, stage] = -5.0 * np.eye(nu)
    return bad


# ------------------------------------------------------------------------------------------------
# The cases of tests/test_blocks_dense_gpu.py, listed here so that tests/test_dense_block_cases.py
# pins the conditioning of exactly the inputs the GPU tolerances rest on.
SEED_COSTATES, SEED_LQR, SEED_DDP = 11, 12, 13
COSTATE_NX = tuple(range(1, 9))
# stages per lane of the parallel scan: N <= 63: 0 or 1; 64: 1; 65: 2 / 1; 130: 3 / 2; 200: 4 / 3
COSTATE_N = (1, 2, 63, 64, 65, 130, 200)
COSTATE_B = 3
COSTATE_WIDE = (4, 70, 65)                 # (nx, N, B): a second 64-thread block of the sequential kernel
LQR_SHAPES = ((2, 1), (4, 1), (3, 2), (8, 4), (5, 8), (8, 8), (1, 1))
LQR_SIZES = ((37, 7), (1, 1))              # (N, B): 259 threads -> block 1 starts inside trajectory 6
DDP_SHAPES = ((2, 1), (4, 1), (8, 4))
DDP_N = (1, 65, 200)
DDP_REG = (0.0, 1e-3, 25.0)                # reg_param of rows 0, 1, 2
DDP_WIDE = (8, 4, 5, 66)                   # (nx, nu, N, B): rows 64, 65 in block 1, a 62-thread tail
DDP_BAD = ((4, 1), (8, 4))                 # N = 20, B = 3, reg_param 0, row 1 poisoned at stage 7
DDP_BAD_N = 20


def costate_case(nx, N, B=COSTATE_B):
    return dense_case(nx, 1, N, B, SEED_COSTATES)


def lqr_case(nx, nu, N, B):
    """(case, lam): lam any randn (B, N+1, nx)"""
    lam = np.random.default_rng([SEED_LQR, nx, nu, N, B]).normal(size=(B, N + 1, nx))
    return dense_case(nx, nu, N, B, SEED_LQR), lam


def ddp_case(nx, nu, N, B=3):
    """(case, reg_param (B,)): DDP_REG repeated over the rows"""
    return dense_case(nx, nu, N, B, SEED_DDP), np.resize(np.asarray(DDP_REG), B)


def ddp_bad_case(nx, nu):
    """(clean case, poisoned case, reg_param): row 1 of the second has cuu[7] = -5 I"""
    case = dense_case(nx, nu, DDP_BAD_N, 3, SEED_DDP)
    return case, poison_row(case, 1, 7), np.zeros(3)
