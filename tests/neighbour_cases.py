"""Batches on which the scan's pivoting fallback runs for SOME trajectories of a wave (test
infrastructure shared by tests/test_kkt_neighbours.py, CPU, and tests/test_kkt_neighbours_gpu.py).

A combine of the reverse scan solves with X = I + C1 J2 by elimination without row exchanges and
redoes it with pivoting if a pivot fails the threshold test (csrc/small_linalg.h lu_np_solve).
With lanes < 64 one wave holds several trajectories, so whether a trajectory's combines are
redone must not depend on its wave-mates.  Each case below is a seeded rand_lq batch in which
(kernel_model.phase2_pivot_census, the CPU model of the pivot decision)
  * some wave holds, at one tree level, a trajectory with a FAILING combine and a wave-mate with a
    combine that passes although partial pivoting would exchange its rows -- and that wave-mate
    fails nowhere itself (so masking every failing trajectory leaves it in the batch),
  * some trajectory of the batch fails nowhere (the control).
The seeds were found by scanning with a margin on both sides of the device's threshold (FAIL_TAU,
PASS_TAU, SWAP_RATIO), so rounding differences between numpy and the device cannot move a
classified combine across it.  The model is a precondition on the inputs, never an oracle for the
device's path.
"""
import numpy as np

import kernel_model as KM
from lq_cases import rand_lq

FAIL_TAU = 0.45    # "fails": |pivot| < 0.45 colmax at some step (the device's threshold is 0.5)
PASS_TAU = 0.55    # "passes": every |pivot| >= 0.55 colmax
SWAP_RATIO = 1.1   # "would swap": an entry below the pivot is larger than 1.1 |pivot|

# (nx, nu, N, lanes, B, seed); affine terms on every second case (AFFINE below).  B = 9 at
# lanes = 8 is one full wave plus a lone trajectory; N = 7 < lanes leaves empty chunks.
CASES = [
    (4, 1, 7, 8, 9, 1), (4, 1, 19, 8, 5, 1), (4, 1, 37, 16, 9, 1), (4, 1, 7, 16, 5, 2),
    (4, 1, 19, 32, 9, 2), (4, 1, 37, 32, 5, 8),
    (8, 4, 7, 8, 9, 1), (8, 4, 19, 8, 5, 6), (8, 4, 37, 16, 9, 4), (8, 4, 7, 16, 5, 3),
    (8, 4, 19, 32, 9, 23), (8, 4, 37, 32, 5, 165),
]
AFFINE = {case: bool(i % 2) for i, case in enumerate(CASES)}
IDS = ["%dx%d-N%d-L%d-B%d-s%d" % case for case in CASES]


def make_case(case):
    nx, nu, N, lanes, B, seed = case
    return rand_lq(seed, B, N, nx, nu, affine=AFFINE[case])


def census(data, b, lanes, tau=0.5, ratio=1.0):
    """phase2_pivot_census of trajectory b of a rand_lq-style batch."""
    g = lambda k: None if k not in data else data[k][b]
    return KM.phase2_pivot_census(data["A"][b], data["B"][b], data["Q"][b], data["R"][b],
                                  data["M"][b], data["r"][b], data["P"][b], data["reg"][b],
                                  g("q"), g("c"), g("p"), L=lanes, tau=tau, ratio=ratio)


def classify(case, data=None):
    """-> (failing, clean, witnesses): the trajectories with a failing combine (FAIL_TAU), those
    that pass everywhere (PASS_TAU), and the (wave, level, failing trajectory, clean wave-mate
    with a passing-but-swapped combine at that level) tuples.  Wave w holds the trajectories
    w * (64 / lanes) .. (w + 1) * (64 / lanes) - 1."""
    nx, nu, N, lanes, B, seed = case
    data = make_case(case) if data is None else data
    fail = [census(data, b, lanes, tau=FAIL_TAU) for b in range(B)]
    safe = [census(data, b, lanes, tau=PASS_TAU, ratio=SWAP_RATIO) for b in range(B)]
    failing = [b for b in range(B) if sum(f for f, _ in fail[b]) > 0]
    clean = [b for b in range(B) if sum(f for f, _ in safe[b]) == 0]
    per = 64 // lanes
    witnesses = []
    for w in range((B + per - 1) // per):
        mates = range(w * per, min(B, (w + 1) * per))
        for lev in range(len(fail[0])):
            witnesses += [(w, lev, f, m) for f in mates for m in mates
                          if fail[f][lev][0] > 0 and m in clean and safe[m][lev][1] > 0]
    return failing, clean, witnesses


def golden_blocks(tag):
    """The committed real Newton blocks (tests/golden): cart200 (golden_v2: two cart-pole N = 200
    trajectories, reg = ||cu||) or cart20 (golden_v1: one cart-pole N = 20 linearisation)."""
    import os
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    g = np.load(os.path.join(here, "golden_v2.npz" if tag == "cart200" else "golden_v1.npz"),
                allow_pickle=False)
    data = {k: g[f"{tag}/{k}"] for k in ("A", "B", "Q", "R", "M", "r", "P")}
    if tag == "cart200":
        data["reg"] = g[f"{tag}/reg"]
    else:
        data = {k: v[None] for k, v in data.items()}
        data["reg"] = np.array([float(np.linalg.norm(g[f"{tag}/cu"]))])
    return data
