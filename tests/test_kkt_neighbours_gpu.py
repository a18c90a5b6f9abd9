"""A trajectory's KKT step must not depend on the trajectories that share its wave.

With lanes < 64 one wave of the scan holds 64 / lanes trajectories.  A combine of the reverse scan
first eliminates X = I + C1 J2 without row exchanges (csrc/small_linalg.h lu_np_solve) and accepts
the result if every pivot passes a threshold test; if ANY lane of the wave fails it
(combine_sklansky votes with __any, over the wave), every lane re-fetches the partner and redoes
the solve with the pivoting elimination lu_pp_solve.  So a trajectory whose combines all pass goes
through the pivoting solve whenever a wave-mate's combine fails.  lu_pp_solve used to pivot
partially: it exchanged rows for such a trajectory (a pivot that passes the threshold need not be
the column's largest entry), and its dx, du, K, d, S, v, pred differed in the last bits between a
batched and a solo solve, between batch orders and under the `active` mask.  On that kernel
(MI355X) 70 of this file's 82 tests failed, by 2e-16 .. 7e-16
in K and what follows from it: batch-equals-solo (with and without gains), mask, tiled and
bwd_pass on all twelve cases of neighbour_cases.CASES ((4, 1) and (8, 4), lanes 8 / 16 / 32), the
order test on ten (the two B = 5, lanes = 8 batches are one wave whatever the order, so the vote
sees the same trajectories); the ten controls (lanes 64, 128, 1) passed.  Now lu_pp_solve pivots
by lu_np_solve's own threshold: it keeps the diagonal wherever that test accepts it, so on a
matrix that passes it repeats lu_np_solve's operations bit for bit, and a lane's combine is a
function of its own operands.  Every comparison here is torch.equal.  (Redoing the solve only in
the lanes whose own test failed, `if (!ok)` around the second solve, was tried instead and is NOT
equivalent in practice: on the (8, 4), N = 19, lanes 32 case it returned K wrong by O(1) for every
trajectory of a wave with a failing combine at level 3, solo solves included -- cause not found;
the accuracy asserts below are what caught it.)

The batches (tests/neighbour_cases.py) are rand_lq data chosen so that, by the CPU model of the
pivot decision, a wave mixes a failing combine with a passing one that partial pivoting would
swap (tests/test_kkt_neighbours.py asserts it).  Every solve is also held to the oracle at
RTOL = 1e-10, so determinism is not bought with accuracy.

The interior-point paths get no such test: the only registered nx = 4 family of
tests/custom_families.py, cartpole_track_limit, produces no failing combine on the linearised
blocks of its first Newton steps (tests/test_kkt_neighbours.py, the census of
test_track_limit_family_newton_blocks_never_fail), so its solves never reach the fallback.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import neighbour_cases as NC  # noqa: E402
from lq_cases import oracle_batch  # noqa: E402

pytestmark = pytest.mark.gpu
RTOL = 1e-10
FIELDS = ("dx", "du", "K", "d", "S", "v", "pred", "feasible")
IN_KEYS = ("A", "B", "Q", "R", "M", "r", "P", "reg", "x0", "q", "c", "p")

_cache = {}


def _case(case):
    """(host data, oracle, device tensors) of a case, computed once and left unchanged."""
    if case not in _cache:
        data = NC.make_case(case)
        dev = {k: torch.as_tensor(np.ascontiguousarray(v), dtype=torch.float64, device="cuda")
               for k, v in data.items()}
        _cache[case] = (data, oracle_batch(data), dev)
    return _cache[case]


def _rows(dev, rows):
    rows = [int(b) for b in rows]
    return {k: v[rows].contiguous() for k, v in dev.items()}


def _solve(dev, lanes, **kw):
    from noc import lqt
    g = dev.get
    res = lqt.kkt_solve(g("A"), g("B"), g("Q"), g("R"), g("M"), g("r"), g("P"), reg=g("reg"),
                        x0=g("x0"), q=g("q"), c=g("c"), p=g("p"), lanes=lanes, **kw)
    return res._asdict()


def _relerr(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(1.0, float(np.max(np.abs(b)))))


def _accurate(out, ref, rows=None, fields=FIELDS):
    for k in fields:
        if out.get(k) is None:
            continue
        got = out[k].cpu().numpy()
        want = ref[k] if rows is None else ref[k][rows]
        if k == "feasible":
            assert np.array_equal(got.astype(bool), want.astype(bool))
        else:
            assert _relerr(got, want) < RTOL, (k, _relerr(got, want))


def _same(got, want, where):
    """Bitwise equality of every field both results carry."""
    for k in FIELDS:
        if want.get(k) is None:
            assert got.get(k) is None, k
            continue
        assert torch.equal(got[k], want[k]), (k, where, float((got[k] - want[k]).abs().max()))


def _batch_equals_solo(case, lanes, **kw):
    nx, nu, N, _, B, seed = case
    data, ref, dev = _case(case)
    full = _solve(dev, lanes, **kw)
    _accurate(full, ref)
    for b in range(B):
        solo = _solve(_rows(dev, [b]), lanes, **kw)
        _same({k: (None if v is None else v[b:b + 1]) for k, v in full.items()}, solo, b)


@pytest.mark.parametrize("case", NC.CASES, ids=NC.IDS)
def test_batch_rows_equal_solo_solves(case):
    _batch_equals_solo(case, case[3], want_value=True)


@pytest.mark.parametrize("case", NC.CASES, ids=NC.IDS)
def test_batch_rows_equal_solo_solves_without_gains(case):
    """want_gains=False: dx, du, pred, feasible (and K, d where they do not stay on chip)."""
    _batch_equals_solo(case, case[3], want_gains=False)


@pytest.mark.parametrize("case", NC.CASES, ids=NC.IDS)
def test_row_order_does_not_matter(case):
    """The reversed batch and a seeded permutation: row perm[i] of the plain solve is row i of
    the permuted one (other wave-mates, other lanes of the wave)."""
    nx, nu, N, lanes, B, seed = case
    data, ref, dev = _case(case)
    plain = _solve(dev, lanes, want_value=True)
    _accurate(plain, ref)
    shuffled = np.random.default_rng(1000 + seed).permutation(B)
    assert not np.array_equal(shuffled, np.arange(B))
    for perm in (np.arange(B)[::-1].copy(), shuffled):
        out = _solve(_rows(dev, perm), lanes, want_value=True)
        _accurate(out, ref, rows=perm)
        idx = torch.as_tensor(perm, device="cuda")
        _same(out, {k: v[idx] for k, v in plain.items()}, list(perm))


@pytest.mark.parametrize("case", NC.CASES, ids=NC.IDS)
def test_masking_the_failing_trajectories_leaves_their_wave_mates_unchanged(case):
    """Every trajectory with a failing combine masked off by `active`: the others' rows equal the
    unmasked solve (among them the wave-mates whose passing combines pivoting would swap), the
    masked rows keep their pre-filled values."""
    from noc import lqt
    nx, nu, N, lanes, B, seed = case
    data, ref, dev = _case(case)
    failing, clean, witnesses = NC.classify(case, data)
    plain = _solve(dev, lanes, want_value=True)
    f64 = dict(dtype=torch.float64, device="cuda")
    shapes = dict(dx=(B, N + 1, nx), du=(B, N, nu), pred=(B,), K=(B, N, nu, nx), d=(B, N, nu),
                  S=(B, N + 1, nx, nx), v=(B, N + 1, nx))
    out = lqt.KKTResult(**{k: torch.full(s, 7.0, **f64) for k, s in shapes.items()},
                        feasible=torch.full((B,), 7, dtype=torch.int32, device="cuda"))
    active = torch.ones(B, dtype=torch.int32, device="cuda")
    active[failing] = 0
    got = _solve(dev, lanes, want_value=True, active=active, out=out)
    kept = [b for b in range(B) if b not in failing]
    assert kept and {m for _, _, _, m in witnesses} <= set(kept)
    _same({k: v[kept] for k, v in got.items()}, {k: v[kept] for k, v in plain.items()}, kept)
    _accurate({k: v[kept] for k, v in got.items()}, ref, rows=kept)
    for k in FIELDS:
        assert bool(torch.all(got[k][failing] == 7)), k


@pytest.mark.parametrize("case", NC.CASES, ids=NC.IDS)
def test_tiled_layout_rows_equal_solo_and_reordered_solves(case):
    """The same through to_tiled / kkt_solve_tiled (x0 is the only affine input of that entry
    point).  K, d are compared after untile: the padding slots are never written."""
    from noc import lqt
    nx, nu, N, lanes, B, seed = case
    data, _, dev = _case(case)
    keys = [k for k in ("A", "B", "Q", "R", "M", "r", "P", "reg", "x0") if k in data]
    ref = oracle_batch({k: data[k] for k in keys})

    def solve(rows):
        d = _rows(dev, rows)
        tb = lqt.to_tiled(*(d[k] for k in ("A", "B", "Q", "R", "M", "r", "P")), lanes)
        res = lqt.kkt_solve_tiled(tb, reg=d["reg"], x0=d.get("x0"), want_value=True)._asdict()
        res["K"] = lqt.untile(res["K"], (len(rows), N, nu, nx), lanes)
        res["d"] = lqt.untile(res["d"], (len(rows), N, nu), lanes)
        _accurate(res, ref, rows=rows)
        return res

    full = solve(list(range(B)))
    for b in range(B):
        _same({k: v[b:b + 1] for k, v in full.items()}, solve([b]), b)
    for perm in (list(range(B))[::-1], list(np.random.default_rng(1000 + seed).permutation(B))):
        idx = torch.as_tensor(perm, device="cuda")
        _same(solve(perm), {k: v[idx] for k, v in full.items()}, perm)


@pytest.mark.parametrize("case", NC.CASES, ids=NC.IDS)
def test_bwd_pass_rows_equal_solo_solves(case):
    from noc import lqt
    nx, nu, N, lanes, B, seed = case
    data, ref, dev = _case(case)
    names = ("K", "d", "S", "v", "pred", "feasible")

    def bwd(d):
        g = d.get
        return dict(zip(names, lqt.bwd_pass(g("A"), g("B"), g("Q"), g("R"), g("M"), g("r"), g("P"),
                                            reg=g("reg"), q=g("q"), c=g("c"), p=g("p"), lanes=lanes)))
    full = bwd(dev)
    _accurate(full, ref, fields=names)
    for b in range(B):
        _same({k: v[b:b + 1] for k, v in full.items()}, bwd(_rows(dev, [b])), b)


CONTROLS = [(NC.CASES[i], lanes) for i in (0, 5, 7, 10) for lanes in (64, 128, 1)
            if not (lanes == 128 and NC.CASES[i][0] == 8)]  # two-wave segments: nx <= 4


@pytest.mark.parametrize("case,lanes", CONTROLS,
                         ids=["%s-at-L%d" % (NC.IDS[NC.CASES.index(c)], L) for c, L in CONTROLS])
def test_controls_one_trajectory_per_wave_and_group_solve(case, lanes):
    """lanes = 64 / 128: a wave (or a pair) per trajectory, so the vote has no neighbours; lanes =
    1: the group solve, which has no combine.  These held before the kernel change as well: the
    harness itself (row slicing, contiguity, launch shapes of a one-row batch) is exact."""
    _batch_equals_solo(case, lanes, want_value=True)
