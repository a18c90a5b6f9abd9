"""The KKT step's `feasible` flag, and what an infeasible, singular or NaN trajectory does to the
trajectories that share its wave.

feasible[b] = all_k Quu_k > 0 steers the interior-point loops (0: retry with a larger
regularisation), and include/noc_hip.h promises that numerical trouble is data, never an error.
In the stand-alone KKT kernels the flag comes from the LDL' pivots of Quu at every stage
(csrc/small_linalg.h ldl_solve; phase 3 of the scan, the group solves), the AND over the L lanes
of a trajectory (segment_sum_and<LW>, which at L < 64 must stay inside the segment) and, at lanes =
128, wave 1's flag handed to lane 0 of wave 0 through LDS (join[PO + 1]).

The batches (tests/feasibility_cases.py) interleave clean rows with rows planted at one stage
each -- the first and last stage, both sides of the first lane boundary, a middle lane, the last
non-empty lane, each wave of a two-wave segment and the join boundary -- with a Quu that is
negative definite (`neg`), indefinite with a unit diagonal and only the third (`mid_pivot`) or only
the last (`last_pivot`) LDL' pivot negative, exactly zero (`zero`: the step contains 1/0) or NaN
(`nan`).  tests/test_feasibility_cases.py holds, on the CPU, that the inputs are what they claim,
with margins (0.1 on the planted pivots, 1e-3 on everything clean).

  a. the flags are [1, 0, 1, 0, ..., 1] through kkt_solve (with and without gains), bwd_pass, the
     tiled entry point and the batch-aware lanes = 0;
  b. the clean rows are bit for bit what they are with the planted rows masked off, as a batch of
     their own and solved alone, and within RTOL of the oracle;
  c. a planted row's K, d, S, v at the stages after the planted one match the clean oracle (they
     do not depend on it); nothing at or before it is compared (LDL' without pivoting on an
     indefinite Quu need not match the oracle's solve); `zero` and `nan` give a non-finite pred
     and no error;
  d. the same through the compact scan (kkt_scan_compact_*) on first-Newton-step blocks of the
     cart-pole and the pendulum.

Only the KKT step kernels see non-finite data here, never a whole-solve driver.  Their addresses
and loop bounds depend on N, L and the chunk lengths alone (lu_pp_solve pivots with selects in
registers), so such data cannot move an access.

The only tolerance is the project's RTOL = 1e-10 (normwise, as tests/test_kkt_gpu.py).
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import feasibility_cases as FC  # noqa: E402
from lq_cases import oracle_batch  # noqa: E402

pytestmark = pytest.mark.gpu
RTOL = 1e-10
CLEAN_MARGIN = 1e-3
FIELDS = ("dx", "du", "K", "d", "S", "v", "pred", "feasible")
BLOCKS = ("A", "B", "Q", "R", "M", "r", "P")
TILED_CASES = [c for c in FC.CASES if c[2] != 1 or c[:2] == (8, 4)]  # grouped layout: (8, 4) only
TILED_IDS = [i for c, i in zip(FC.CASES, FC.IDS) if c in TILED_CASES]


def relerr(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(1.0, float(np.max(np.abs(b)))))


def _dev(data):
    return {k: torch.as_tensor(np.ascontiguousarray(v), dtype=torch.float64, device="cuda")
            for k, v in data.items()}


def _rows(dev, rows):
    rows = [int(b) for b in rows]
    return {k: v[rows].contiguous() for k, v in dev.items()}


def _solve(dev, lanes, **kw):
    from noc import lqt
    g = dev.get
    res = lqt.kkt_solve(g("A"), g("B"), g("Q"), g("R"), g("M"), g("r"), g("P"), reg=g("reg"),
                        x0=g("x0"), q=g("q"), c=g("c"), p=g("p"), lanes=lanes, **kw)
    return res._asdict()


def _flags(t):
    return [int(f) for f in t.cpu().numpy()]


def _same(got, want, where):
    """Bitwise equality of every field (NaN never occurs in a clean row, so torch.equal is it)."""
    for k in FIELDS:
        assert got[k] is not None and want[k] is not None, k
        assert torch.equal(got[k], want[k]), (k, where, float((got[k] - want[k]).abs().max()))


@functools.lru_cache(maxsize=None)
def clean_ref(nx, nu, L, N, affine):
    """The oracle's solve of the unplanted batch (shared by the kinds; never modified)."""
    return oracle_batch(FC.batch(nx, nu, N, L, None, FC.seed_of(nx, nu, L, N), affine)[0])


@functools.lru_cache(maxsize=None)
def made(case):
    """One case, computed once and shared (never modified): the batch, its device copy and the
    fused solve with gains and value function at the case's lanes -- one launch, then a
    synchronize, which must raise nothing whatever the planted rows hold."""
    nx, nu, L, N, affine, kind = case
    data, planted, clean, flags = FC.batch(nx, nu, N, L, kind, FC.seed_of(nx, nu, L, N), affine)
    dev = _dev(data)
    full = _solve(dev, L, want_value=True)
    torch.cuda.synchronize()
    return dict(data=data, planted=planted, clean=clean, flags=[int(f) for f in flags], dev=dev,
                full=full, pos=FC.positions(N, L), ref=clean_ref(nx, nu, L, N, affine))


# ---- a. the flags, through every entry point ---------------------------------------------------
@pytest.mark.parametrize("case", FC.CASES, ids=FC.IDS)
def test_flags_fused_solve(case):
    m = made(case)
    assert _flags(m["full"]["feasible"]) == m["flags"]


@pytest.mark.parametrize("case", FC.CASES, ids=FC.IDS)
def test_flags_without_gains(case):
    """want_gains=False: K, d stay in LDS wherever gains_on_chip says so."""
    from noc import lqt
    nx, nu, L, N, affine, kind = case
    m = made(case)
    out = _solve(m["dev"], L, want_gains=False)
    torch.cuda.synchronize()
    assert (out["K"] is None) == lqt.gains_on_chip(nx, nu, N, L) == (out["d"] is None)
    assert _flags(out["feasible"]) == m["flags"]


@pytest.mark.parametrize("case", FC.CASES, ids=FC.IDS)
def test_flags_bwd_pass(case):
    from noc import lqt
    m = made(case)
    g = m["dev"].get
    res = lqt.bwd_pass(g("A"), g("B"), g("Q"), g("R"), g("M"), g("r"), g("P"), reg=g("reg"),
                       q=g("q"), c=g("c"), p=g("p"), lanes=case[2])
    torch.cuda.synchronize()
    assert _flags(res[5]) == m["flags"]


@pytest.mark.parametrize("case", TILED_CASES, ids=TILED_IDS)
def test_flags_tiled(case):
    """to_tiled + kkt_solve_tiled (x0 is that entry point's only affine input; Quu sees none)."""
    from noc import lqt
    m = made(case)
    d = m["dev"]
    tb = lqt.to_tiled(*(d[k] for k in BLOCKS), case[2])
    res = lqt.kkt_solve_tiled(tb, reg=d["reg"], x0=d.get("x0"), want_value=True)
    torch.cuda.synchronize()
    assert _flags(res.feasible) == m["flags"]


@pytest.mark.parametrize("case", FC.CASES, ids=FC.IDS)
def test_flags_default_lanes(case):
    """lanes = 0: the batch-aware pick.  For these batches (at most 13 rows, far fewer waves than
    the MI355X has SIMDs) it is the group solve at nx = 8, else one wave per trajectory, two from
    N = 128 on (csrc/noc_abi.hip kkt_pick_lanes) -- not the lane count the positions were derived
    for, so the planted stages fall anywhere in its chunks."""
    from noc import lqt
    nx, nu, L, N, affine, kind = case
    m = made(case)
    picked = lqt.pick_lanes(nx, nu, N, len(m["flags"]))
    assert picked == (1 if nx == 8 else 128 if N >= 128 else 64)
    out = _solve(m["dev"], 0, want_value=True)
    torch.cuda.synchronize()
    assert _flags(out["feasible"]) == m["flags"]


# ---- b. the clean rows are untouched -----------------------------------------------------------
@pytest.mark.parametrize("case", FC.CASES, ids=FC.IDS)
def test_clean_rows_do_not_see_the_planted_ones(case):
    from noc import lqt
    nx, nu, L, N, affine, kind = case
    m = made(case)
    planted, clean, dev, full = m["planted"], m["clean"], m["dev"], m["full"]
    Bt = len(m["flags"])
    want = {k: v[clean] for k, v in full.items()}
    for k in FIELDS:
        assert bool(torch.isfinite(want[k]).all()), k
    # the planted rows masked off: they keep the pre-filled 7
    f64 = dict(dtype=torch.float64, device="cuda")
    shapes = dict(dx=(Bt, N + 1, nx), du=(Bt, N, nu), pred=(Bt,), K=(Bt, N, nu, nx), d=(Bt, N, nu),
                  S=(Bt, N + 1, nx, nx), v=(Bt, N + 1, nx))
    out = lqt.KKTResult(**{k: torch.full(s, 7.0, **f64) for k, s in shapes.items()},
                        feasible=torch.full((Bt,), 7, dtype=torch.int32, device="cuda"))
    active = torch.ones(Bt, dtype=torch.int32, device="cuda")
    active[planted] = 0
    got = _solve(dev, L, want_value=True, active=active, out=out)
    _same({k: v[clean] for k, v in got.items()}, want, "masked")
    for k in FIELDS:
        assert bool(torch.all(got[k][planted] == 7)), k
    # the clean rows as a batch of their own, and each alone
    _same(_solve(_rows(dev, clean), L, want_value=True), want, "own batch")
    for i, b in enumerate(clean):
        solo = _solve(_rows(dev, [b]), L, want_value=True)
        _same(solo, {k: v[i:i + 1] for k, v in want.items()}, ("solo", b))
    torch.cuda.synchronize()
    # and they are the solution
    for k in FIELDS:
        got_k, ref_k = want[k].cpu().numpy(), m["ref"][k][clean]
        if k == "feasible":
            assert np.array_equal(got_k.astype(bool), ref_k.astype(bool))
        else:
            assert relerr(got_k, ref_k) < RTOL, (k, relerr(got_k, ref_k))


# ---- c. what a planted row still owes ----------------------------------------------------------
@pytest.mark.parametrize("case", FC.CASES, ids=FC.IDS)
def test_planted_rows_after_the_planted_stage(case):
    nx, nu, L, N, affine, kind = case
    m = made(case)
    full = {k: m["full"][k].cpu().numpy() for k in ("K", "d", "S", "v", "pred", "feasible")}
    for b, s in zip(m["planted"], m["pos"]):
        assert full["feasible"][b] == 0
        for k in ("K", "d", "S", "v"):
            got, ref = full[k][b, s + 1:], m["ref"][k][b, s + 1:]
            if ref.size:  # K, d: nothing after s = N - 1 (S_N, v_N are the terminal cost)
                assert relerr(got, ref) < RTOL, (k, b, s, relerr(got, ref))
        if kind in ("zero", "nan"):
            assert not np.isfinite(full["pred"][b]), (b, s, full["pred"][b])


# ---- d. the compact entry point ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def compact_setup(name, L, N):
    """The compact engine's first-Newton-step blocks (as tests/test_scan_struct_gpu.py), their
    natural copy on the host, the long-double value chains of every row and the unplanted compact
    solve.  Computed once and shared (never modified)."""
    from noc import lqt, problems, _lib
    from noc.ipm import BatchedIPM
    pos = FC.positions(N, L)
    Bt = 2 * len(pos) + 1
    ocp = problems.make_problem(name, N)
    x0s, u0 = problems.initial_conditions(name, N, Bt, seed=FC.COMPACT_SEED)
    engs = {}
    for compact in (True, False):
        e = BatchedIPM(ocp.family, N, Bt, lanes=L, compact=compact)
        assert e.compact is compact
        e.load(u0, x0s)
        e.init(0.1)
        e.prepare(_lib.MODE_PAR, 0)
        engs[compact] = e
    eng = engs[True]
    tc = eng.tiled_blocks()
    assert isinstance(tc, lqt.CompactBlocks) and tc.lanes == L
    nat = eng.natural_blocks()
    nx = nat["A"].shape[-1]
    # the layout the header states for the compact R of both families: width 1, packed E = 1 --
    # the tiled layout of the natural R itself.  Held on the slots that carry a stage, against the
    # dense engine's R (which never went through noc_blocks_expand): tile() leaves the padding
    # slots of its buffer unwritten, so whole buffers cannot be compared.
    assert nat["R"].shape == (Bt, N, 1, 1) and tc.R.numel() == lqt.tiled_numel(N, Bt, L, 1)
    natd_R = engs[False].natural_blocks()["R"]
    assert torch.equal(lqt.untile(tc.R, (Bt, N, 1, 1), L, sym=True), natd_R)
    assert torch.equal(nat["R"], natd_R)
    assert torch.equal(lqt.untile(lqt.tile(natd_R, L, sym=True), (Bt, N, 1, 1), L, sym=True), natd_R)
    x0 = torch.as_tensor(np.random.default_rng(13).normal(size=(Bt, nx)) * 0.1, device="cuda")
    reg = eng.t["reg"].clone()
    plain = lqt.kkt_solve_tiled(tc, reg=reg, x0=x0, want_value=True)
    torch.cuda.synchronize()
    case = {k: nat[k].cpu().numpy() for k in BLOCKS}
    case["reg"] = reg.cpu().numpy()
    chains = [FC.value_chain(case, b, 0) for b in range(Bt)]
    for b in range(Bt):  # every row is clean here, with the margin of the CPU precondition test
        lam = min(float(np.linalg.eigvalsh(np.asarray(q, dtype=np.float64)).min())
                  for q in chains[b][0].values())
        assert lam >= CLEAN_MARGIN, (b, lam)
    assert _flags(plain.feasible) == [1] * Bt
    return dict(eng=eng, tc=tc, nat=nat, x0=x0, reg=reg, plain=plain, case=case, chains=chains,
                pos=pos, Bt=Bt, nx=nx)


@pytest.mark.parametrize("kind", FC.COMPACT_KINDS)
@pytest.mark.parametrize("name,L,N", FC.COMPACT_GRID)
def test_compact_scan_flags_and_clean_rows(name, L, N, kind):
    from noc import lqt
    s_ = compact_setup(name, L, N)
    pos, Bt, nx, tc, plain = s_["pos"], s_["Bt"], s_["nx"], s_["tc"], s_["plain"]
    planted = [2 * i + 1 for i in range(len(pos))]
    clean = [2 * i for i in range(len(pos) + 1)]
    case = {k: v.copy() for k, v in s_["case"].items()}
    for b, s in zip(planted, pos):
        FC.plant(case, b, s, kind, s_["chains"][b][1][s + 1])
        if kind == "neg":  # the planted Quu, from the blocks the device solves
            quu = float(case["R"][b, s, 0, 0] + case["reg"][b] +
                        np.asarray(case["B"][b, s].T @ np.asarray(s_["chains"][b][1][s + 1], float)
                                   @ case["B"][b, s]).item())
            assert abs(quu + 2.0) < 1e-9, (b, s, quu)
    R = torch.as_tensor(case["R"], device="cuda")
    tcp = tc._replace(R=lqt.tile(R, L, sym=True))
    td = lqt.to_tiled(*(R if k == "R" else s_["nat"][k] for k in BLOCKS), L)
    rc = lqt.kkt_solve_tiled(tcp, reg=s_["reg"], x0=s_["x0"], want_value=True)
    rd = lqt.kkt_solve_tiled(td, reg=s_["reg"], x0=s_["x0"], want_value=True)
    torch.cuda.synchronize()
    expected = [0 if b in planted else 1 for b in range(Bt)]
    assert _flags(rc.feasible) == _flags(rd.feasible) == expected
    if kind == "nan":
        assert not bool(torch.isfinite(rc.pred[planted]).any())
    shapes = dict(K=(Bt, N, 1, nx), d=(Bt, N, 1))
    for res, tag in ((rc, "compact"), (rd, "dense")):
        for k in FIELDS:
            got, want = getattr(res, k), getattr(plain, k)
            if k in shapes:
                got, want = lqt.untile(got, shapes[k], L), lqt.untile(want, shapes[k], L)
            assert torch.equal(got[clean], want[clean]), (tag, k)
