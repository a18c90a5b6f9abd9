"""Batches with a planted infeasible stage for the KKT step's `feasible` flag (test infrastructure
shared by tests/test_feasibility_cases.py, CPU, and tests/test_kkt_feasibility_gpu.py).

feasible[b] = all_k Quu_k > 0 (include/noc_hip.h) comes, in the stand-alone KKT kernels, from the
LDL' pivots of Quu at every stage (csrc/small_linalg.h ldl_solve), ANDed over the L lanes of the
trajectory (segment_sum_and<LW>) and, at lanes = 128, joined across the two waves through LDS.

plant(case, b, s, kind) edits trajectory b of a rand_lq-style batch at stage s in place so that
Quu_s = R_s + reg_b I + B_s' S_{s+1} B_s is a chosen matrix T.  S_{s+1} depends on the stages after
s only, so it is computed by the sequential Riccati recursion on the (still clean) data, in
np.longdouble, and R_s := T - reg_b I - B_s' S_{s+1} B_s.  Kinds:
  neg         T = -2 I                                        (any nu)
  mid_pivot   T = (1 - a) I + a 11', a = -0.6   (nu = 4): unit diagonal, LDL' pivots
              1, 0.64, -0.8, 6.4 -- only the THIRD is negative, the last is positive again
  last_pivot  the same form, a = -0.4           (nu = 4): pivots 1, 0.84, 0.4667, -1.4 -- the
              diagonal and every leading 3 x 3 minor are positive
  zero        B_s := 0, R_s := -reg_b I: the device forms Quu_s = (R + reg) + 0 = 0.0 exactly (M_s
              stays non-zero), so the step contains 1/0; the contract is flag 0, non-finite values,
              no error
  nan         R_s[0, 0] := NaN
positions(N, L) are the stages to plant at, from the chunk map of include/noc_hip.h (lanes
l < N % L own N/L + 1 stages, the others N/L; chunks are contiguous in time).
batch(...) interleaves clean and planted rows, so every wave at L < 64 and every group-solve wave
mixes both, and a flag that leaks one row over, or a missed position, shows as a wrong entry of
[1, 0, 1, 0, ..., 1].

This module is a recipe for inputs, never an oracle for the device's path.
"""
import functools

import numpy as np

from lq_cases import rand_lq

LD = np.longdouble
KINDS = ("neg", "mid_pivot", "last_pivot", "zero", "nan")
TARGET_A = {"mid_pivot": -0.6, "last_pivot": -0.4}
# LDL' pivots of (1 - a) I + a 11' (n = 4): d_j = (1 - a)(1 + j a) / (1 + (j - 1) a), j = 1..3
PIVOTS = {"neg": None, "mid_pivot": (1.0, 0.64, -0.8, 6.4),
          "last_pivot": (1.0, 0.84, 0.392 / 0.84, -1.4)}

SHAPES = ((2, 1), (4, 1), (8, 4))


def horizons(nx, L):
    """The horizons of the GPU tests at L lanes: L - 1 leaves the last lane empty (its identity
    flag 1 must not mask, or be masked by, the others), 2 L + 3 gives ragged chunks of 3 and 2;
    two-wave segments (nx <= 4): wave 1 empty, partly filled (N < L), two-stage chunks."""
    if L == 128:
        return (40, 100, 150) if nx <= 4 else ()
    if L == 1:
        return (7, 37)
    return (L - 1, 2 * L + 3)


def kinds_for(nu):
    return tuple(k for k in KINDS if nu == 4 or k not in TARGET_A)


# (nx, nu, L, N, affine): affine terms on every second case
GRID = [(nx, nu, L, N) for nx, nu in SHAPES for L in (8, 16, 32, 64, 128, 1)
        for N in horizons(nx, L)]
GRID = [g + (bool(i % 2),) for i, g in enumerate(GRID)]
# (nx, nu, L, N, affine, kind)
CASES = [g + (kind,) for g in GRID for kind in kinds_for(g[1])]
IDS = ["%dx%d-L%d-N%d-%s-%s" % (c[0], c[1], c[2], c[3], "aff" if c[4] else "lin", c[5])
       for c in CASES]


# the compact entry point (kkt_scan_compact_*): first-Newton-step blocks of the built-in families
# (problems.initial_conditions(name, N, 2 len(positions) + 1, COMPACT_SEED), bp = 0.1), planted
# through the natural R like the rand_lq batches
COMPACT_SEED = 11
COMPACT_GRID = [(name, L, N) for name in ("cartpole", "pendulum") for L in (8, 32)
                for N in (L - 1, 2 * L + 3)]
COMPACT_KINDS = ("neg", "nan")


def seed_of(nx, nu, L, N):
    """One seed per (shape, L, N): the clean data (and so its oracle) is shared by every kind."""
    return 9000 + 100 * nx + 7 * L + N


def _chunks(N, L):
    base, rem = divmod(N, L)
    lens = [base + (1 if l < rem else 0) for l in range(L)]
    starts = [l * base + min(l, rem) for l in range(L)]
    return starts, lens


def positions(N, L, claims=False):
    """Stages to plant at, each once, in the order listed below.  claims=True: (stage, lane)
    pairs -- the lane of the L-lane segment that the position is meant to hit.
      L in 8..64: s = 0; s = N - 1; the last stage of lane 0's chunk; the first stage of lane 1's
                  chunk; a middle stage of a middle non-empty lane; the single or last stage of
                  the last non-empty lane (chunks are contiguous, so that is N - 1 again: listed
                  once)
      L = 128:    a stage of wave 0 (lanes < 64), a stage of wave 1 in a lane that is not the
                  wave's first, the first stage of wave 1 (the join boundary); the wave-1 entries
                  only where wave 1 owns a stage
      L = 1:      0, N // 2, N - 1 (the group solve has no chunk map: lane 0)"""
    if L == 1:
        out = [(0, 0), (N // 2, 0), (N - 1, 0)]
    else:
        starts, lens = _chunks(N, L)
        full = [l for l in range(L) if lens[l] > 0]
        if L == 128:
            w0 = [l for l in full if l < 64]
            w1 = [l for l in full if l >= 64]
            m = w0[len(w0) // 2]
            out = [(starts[m] + lens[m] // 2, m)]
            if w1:
                m = w1[len(w1) // 2]
                out += [(starts[m] + lens[m] // 2, m), (starts[64], 64)]
        else:
            m = full[len(full) // 2]
            out = [(0, 0), (N - 1, full[-1]), (starts[0] + lens[0] - 1, 0)]
            if len(full) > 1:
                out.append((starts[1], 1))
            out += [(starts[m] + lens[m] // 2, m), (starts[full[-1]] + lens[full[-1]] - 1, full[-1])]
    seen, uniq = set(), []
    for s, l in out:
        if s not in seen:
            seen.add(s)
            uniq.append((s, l))
    return uniq if claims else [s for s, _ in uniq]


def _solve_ld(Amat, Bmat):
    """Amat^-1 Bmat in long double (elimination with partial pivoting; np.linalg would drop to
    fp64)."""
    n = Amat.shape[0]
    A = np.array(Amat, dtype=LD)
    X = np.array(Bmat, dtype=LD).reshape(n, -1)
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if p != k:
            A[[k, p]] = A[[p, k]]
            X[[k, p]] = X[[p, k]]
        for i in range(k + 1, n):
            f = A[i, k] / A[k, k]
            A[i, k:] -= f * A[k, k:]
            X[i] -= f * X[k]
    for k in range(n - 1, -1, -1):
        X[k] = (X[k] - A[k, k + 1:] @ X[k + 1:]) / A[k, k]
    return X.reshape(np.shape(Bmat))


def value_chain(case, b, down_to):
    """The sequential Riccati recursion (S:42-75) of trajectory b in long double over the stages
    N - 1 .. down_to: ({k: Quu_k}, {k: S_k}) with Quu_k = R_k + reg I + B_k' S_{k+1} B_k, k =
    down_to .. N - 1 (S_N = P too).  S_k does not depend on the stages before k."""
    g = lambda k: np.asarray(case[k][b], dtype=LD)
    A, B, Q, R, M = g("A"), g("B"), g("Q"), g("R"), g("M")
    N, nu = B.shape[0], B.shape[2]
    S = g("P")
    reg = LD(case["reg"][b])
    quu, val = {}, {N: S}
    for k in range(N - 1, down_to - 1, -1):
        Quu = R[k] + reg * np.eye(nu, dtype=LD) + B[k].T @ S @ B[k]
        Qxu = M[k] + A[k].T @ S @ B[k]
        quu[k] = Quu
        S = Q[k] + A[k].T @ S @ A[k] - Qxu @ _solve_ld(Quu, Qxu.T)
        S = (S + S.T) / 2
        val[k] = S
    return quu, val


def target(kind, nu):
    if kind == "neg":
        return -2.0 * np.eye(nu)
    if nu != 4:
        raise ValueError("%s needs nu = 4" % kind)
    a = TARGET_A[kind]
    return (1.0 - a) * np.eye(nu) + a * np.ones((nu, nu))


def plant(case, b, s, kind, S_next=None):
    """Edit trajectory b at stage s in place (see the module docstring).  The stages after s of
    that trajectory must still be clean.  S_next: S_{s+1} of the clean data in long double where
    the caller has it already (batch() shares one recursion among the kinds)."""
    nu = case["B"].shape[-1]
    if kind == "nan":
        case["R"][b, s, 0, 0] = np.nan
    elif kind == "zero":
        case["B"][b, s] = 0.0
        case["R"][b, s] = -case["reg"][b] * np.eye(nu)
    else:
        S = value_chain(case, b, s + 1)[1][s + 1] if S_next is None else S_next
        Bs = np.asarray(case["B"][b, s], dtype=LD)
        R = target(kind, nu).astype(LD) - LD(case["reg"][b]) * np.eye(nu, dtype=LD) - Bs.T @ S @ Bs
        case["R"][b, s] = np.asarray((R + R.T) / 2, dtype=np.float64)
    return case


@functools.lru_cache(maxsize=None)
def clean_chains(nx, nu, N, L, seed, affine):
    """value_chain(.., down_to=0) of every row of the unplanted batch, computed once and shared
    (never modified): a list of ({k: Quu_k}, {k: S_k})."""
    case = batch(nx, nu, N, L, None, seed, affine)[0]
    return [value_chain(case, b, 0) for b in range(case["A"].shape[0])]


def batch(nx, nu, N, L, kind, seed, affine):
    """-> (case, planted_rows, clean_rows, expected_flags): a rand_lq batch of
    2 len(positions(N, L)) + 1 rows, odd row 2 i + 1 planted at position i, even rows clean.
    kind=None: the same batch with nothing planted (the rows and flags are still reported as for a
    planted one; every row is then clean)."""
    pos = positions(N, L)
    Bt = 2 * len(pos) + 1
    case = rand_lq(seed, Bt, N, nx, nu, affine=affine)
    planted = [2 * i + 1 for i in range(len(pos))]
    clean = [2 * i for i in range(len(pos) + 1)]
    if kind is not None:
        chains = clean_chains(nx, nu, N, L, seed, affine) if kind in ("neg",) + tuple(TARGET_A) else None
        for i, s in enumerate(pos):
            plant(case, planted[i], s, kind, None if chains is None else chains[planted[i]][1][s + 1])
    flags = np.ones(Bt, dtype=np.int32)
    flags[planted] = 0
    return case, planted, clean, flags
