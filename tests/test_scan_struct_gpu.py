"""GPU checks of the KKT scan's closed-loop structure predicates (BlockStruct::nzF / nzf) and of
the peeled first stage of a chunk in phase 3: the compact scan, the dense scan
and the CPU oracle on the same blocks.

Compact against dense: torch.equal (a skipped product has an exact structural zero as a factor;
the peeled stage assigns what the sums I * F, 0 + I * f give, up to the sign of a zero, which ==
does not see).  Against oracle/noc_oracle.kkt_solve: RTOL = 1e-10, as tests/test_kkt_gpu.py.

Shapes, at batch 3 and lanes 8 and 32, cart-pole and pendulum: N = lanes - 1 (the last lane's chunk
is empty: it keeps Phi = I), N = lanes (one stage per lane: the peeled stage is the only one, and
it is also the one handed to phase 4), N = 2 * lanes + 3 (chunks of 3 and 2 stages, the last lane
shorter than the first).  The pendulum at 32 lanes takes the register-cached chunks for the two
short horizons and the streamed ones for the long one.  MODE_FULL through kkt_solve_tiled;
MODE_BWD followed by MODE_FWD through bwd_pass / fwd_pass, the entry points par_bwd_pass /
par_fwd_pass call (noc_par_bwd_pass, noc_par_fwd_pass: dense natural blocks, no compact form)."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from lq_cases import oracle_batch  # noqa: E402

pytestmark = pytest.mark.gpu
RTOL = 1e-10
FIELDS = ("A", "B", "Q", "R", "M", "r", "P")
B = 3
CASES = [(name, N, L) for name in ("cartpole", "pendulum") for L in (8, 32)
         for N in (L - 1, L, 2 * L + 3)]


def relerr(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(1.0, float(np.max(np.abs(b)))))


@functools.lru_cache(maxsize=None)
def solved(name, N, lanes):
    """One case, computed once and shared (never modified): both engines' blocks, the compact and
    the dense fused solve (with gains, x0 set), the dense backward + forward passes and the
    oracle's solve of the dense blocks."""
    from noc import lqt, problems, _lib
    from noc.ipm import BatchedIPM
    ocp = problems.make_problem(name, N)
    x0s, u0 = problems.initial_conditions(name, N, B, seed=11)
    eng = {}
    for compact in (True, False):
        e = BatchedIPM(ocp.family, N, B, lanes=lanes, compact=compact)
        assert e.compact is compact
        e.load(u0, x0s)
        e.init(0.1)
        e.prepare(_lib.MODE_PAR, 0)
        eng[compact] = e
    ec, ed = eng[True], eng[False]
    nd = ed.natural_blocks()
    nx = nd["A"].shape[-1]
    x0 = torch.as_tensor(np.random.default_rng(13).normal(size=(B, nx)) * 0.1, device="cuda")
    tc = ec.tiled_blocks()
    td = lqt.to_tiled(*(nd[k] for k in FIELDS), lanes)
    assert isinstance(tc, lqt.CompactBlocks) and tc.lanes == lanes
    rc = lqt.kkt_solve_tiled(tc, reg=ec.t["reg"], x0=x0, want_gains=True)
    rd = lqt.kkt_solve_tiled(td, reg=ed.t["reg"], x0=x0, want_gains=True)
    bwd = lqt.bwd_pass(*(nd[k] for k in FIELDS), reg=ed.t["reg"], lanes=lanes)
    fwd = lqt.fwd_pass(nd["A"], nd["B"], bwd[0], bwd[1], x0=x0, lanes=lanes)
    torch.cuda.synchronize()
    case = {k: nd[k].cpu().numpy() for k in FIELDS}
    case["reg"] = ed.t["reg"].cpu().numpy()
    case["x0"] = x0.cpu().numpy()
    return dict(ec=ec, ed=ed, tc=tc, td=td, x0=x0, rc=rc, rd=rd, bwd=bwd, fwd=fwd, case=case,
                ref=oracle_batch(case))


def assert_same_result(rc, rd, tb):
    from noc import lqt
    for k in ("dx", "du", "pred", "feasible"):
        assert torch.equal(getattr(rc, k), getattr(rd, k)), k
    for k, shape in (("K", (tb.Bt, tb.N, tb.nu, tb.nx)), ("d", (tb.Bt, tb.N, tb.nu))):
        assert torch.equal(lqt.untile(getattr(rc, k), shape, tb.lanes),
                           lqt.untile(getattr(rd, k), shape, tb.lanes)), k


@pytest.mark.parametrize("name,N,lanes", CASES)
def test_full_compact_equals_dense(name, N, lanes):
    s = solved(name, N, lanes)
    assert_same_result(s["rc"], s["rd"], s["td"])


@pytest.mark.parametrize("name,N,lanes", CASES)
def test_full_matches_oracle(name, N, lanes):
    s = solved(name, N, lanes)
    ref = s["ref"]
    for tag, res in (("compact", s["rc"]), ("dense", s["rd"])):
        for k in ("dx", "du", "pred"):
            e = relerr(getattr(res, k).cpu().numpy(), ref[k])
            print(f"{name} N={N} L={lanes} {tag} {k}: rel err {e:.3e}")
            assert e < RTOL, (tag, k)
        assert np.array_equal(res.feasible.cpu().numpy().astype(bool), ref["feasible"].astype(bool))


@pytest.mark.parametrize("name,N,lanes", CASES)
def test_bwd_then_fwd_matches_oracle(name, N, lanes):
    s = solved(name, N, lanes)
    ref = s["ref"]
    K, d, _, _, pred, feas = s["bwd"]
    du, dx = s["fwd"]
    for k, t in (("K", K), ("d", d), ("pred", pred), ("du", du), ("dx", dx)):
        e = relerr(t.cpu().numpy(), ref[k])
        print(f"{name} N={N} L={lanes} bwd+fwd {k}: rel err {e:.3e}")
        assert e < RTOL, k
    assert np.array_equal(feas.cpu().numpy().astype(bool), ref["feasible"].astype(bool))


@pytest.mark.parametrize("name,N,lanes", [("cartpole", 19, 8), ("pendulum", 67, 32)])
def test_active_mask_kills_one_trajectory_of_a_wave(name, N, lanes):
    """Trajectory 1 of the three sharing wave 0 is masked off: it keeps what `out` held, the
    others are the compact = dense = oracle results."""
    from noc import lqt
    s = solved(name, N, lanes)
    active = torch.tensor([1, 0, 1], dtype=torch.int32, device="cuda")
    outs = []
    for tb, e in ((s["tc"], s["ec"]), (s["td"], s["ed"])):
        out = lqt.kkt_solve_tiled(tb, reg=e.t["reg"], want_gains=True)  # allocates
        for t in out:
            if t is not None:
                t.fill_(7)
        res = lqt.kkt_solve_tiled(tb, reg=e.t["reg"], x0=s["x0"], active=active, out=out)
        assert res is out
        outs.append(res)
    torch.cuda.synchronize()
    assert_same_result(outs[0], outs[1], s["td"])
    live = [0, 2]
    for res in outs:
        assert bool((res.dx[1] == 7).all()) and bool((res.du[1] == 7).all())
        assert float(res.pred[1]) == 7 and int(res.feasible[1]) == 7
        for k in ("dx", "du", "pred"):
            assert relerr(getattr(res, k)[live].cpu().numpy(), s["ref"][k][live]) < RTOL, k
        assert np.array_equal(res.feasible[live].cpu().numpy().astype(bool),
                              s["ref"]["feasible"][live].astype(bool))
