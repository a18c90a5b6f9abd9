"""GPU checks of the compact (structure-aware) LQ blocks outside the persistent solver: the
stand-alone compact KKT scan (noc_kkt_solve_compact), the compact-writing linearisation
(noc_ipm_prepare_compact), the expand kernel (noc_blocks_expand) and the launch-per-phase loop on
them (noc_ipm_step*_compact).

The yardstick is the dense path, bit for bit (torch.equal): a skipped product with a structural
zero adds an exact zero, and the rebuilt constants are the doubles the dense blocks hold (DESIGN.md
§3.11, §3.12).  Oracle parity (oracle/noc_oracle.kkt_solve) at the KKT tests' RTOL = 1e-10 on top.
Shapes: the smallest that reach every path -- empty chunks (N < L), uneven chunks, cmax = 2 with
one-stage lanes, one stage per lane, the pendulum's register-cached (cmax <= 2 at L >= 32) and
streamed chunks, waves with dead segments (B = 3, 37), and one batch whose waves exceed the SIMDs
(the two-waves-per-SIMD instance the c3 bench launch runs; every smaller batch takes the
one-wave-per-SIMD instance)."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from lq_cases import oracle_batch  # noqa: E402

pytestmark = pytest.mark.gpu
RTOL = 1e-10
FIELDS = ("A", "B", "Q", "R", "M", "r", "P")

CART = [(5, 8), (20, 8), (33, 32), (64, 64), (70, 16)]   # N, lanes
PEND = [(100, 64), (65, 32), (9, 8)]
CASES = [("cartpole", N, L) for N, L in CART] + [("pendulum", N, L) for N, L in PEND]


def relerr(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(1.0, float(np.max(np.abs(b)))))


def engines(name, N, lanes, B, terminal, seed=3):
    """(compact engine, dense engine) after init + prepare on the same seeded inputs"""
    from noc import problems, _lib
    from noc.ipm import BatchedIPM
    ocp = problems.make_problem(name, N)
    x0, u0 = problems.initial_conditions(name, N, B, seed=seed)
    out = []
    for compact in (True, False):
        eng = BatchedIPM(ocp.family, N, B, lanes=lanes, compact=compact)
        assert eng.compact is compact
        eng.load(u0, x0)
        eng.init(0.1)
        eng.prepare(_lib.MODE_PAR, terminal)
        out.append(eng)
    return out


@functools.lru_cache(maxsize=None)
def solved(name, N, lanes, B, terminal):
    """One case, computed once and shared (never modified): the natural blocks of both engines,
    the compact and the dense solve (with gains), and the oracle's solve of the dense blocks."""
    from noc import lqt
    ec, ed = engines(name, N, lanes, B, terminal)
    nc, nd = ec.natural_blocks(), ed.natural_blocks()
    tb = ec.tiled_blocks()
    assert isinstance(tb, lqt.CompactBlocks) and isinstance(ed.tiled_blocks(), lqt.TiledBlocks)
    rc = lqt.kkt_solve_tiled(tb, reg=ec.t["reg"], want_gains=True)
    rd = lqt.kkt_solve_tiled(lqt.to_tiled(*(nd[k] for k in FIELDS), lanes), reg=ed.t["reg"],
                             want_gains=True)
    torch.cuda.synchronize()
    case = {k: nd[k].cpu().numpy() for k in FIELDS}
    case["reg"] = ed.t["reg"].cpu().numpy()
    return dict(ec=ec, ed=ed, nc=nc, nd=nd, rc=rc, rd=rd, case=case, ref=oracle_batch(case))


def assert_same_result(rc, rd, tb, gains=True):
    """tb: the blocks' geometry.  K, d are tiled buffers whose padding (chunk slots without a
    stage) is never written: compared in the natural layout, i.e. on every stage's entries."""
    from noc import lqt
    for k in ("dx", "du", "pred", "feasible"):
        assert torch.equal(getattr(rc, k), getattr(rd, k)), k
    if gains:
        for k, shape in (("K", (tb.Bt, tb.N, tb.nu, tb.nx)), ("d", (tb.Bt, tb.N, tb.nu))):
            a, b = getattr(rc, k), getattr(rd, k)
            assert a is not None and b is not None, k
            assert torch.equal(lqt.untile(a, shape, tb.lanes), lqt.untile(b, shape, tb.lanes)), k


@pytest.mark.parametrize("terminal", [0, 1])
@pytest.mark.parametrize("B", [3, 37])
@pytest.mark.parametrize("name,N,lanes", CASES)
def test_compact_equals_dense_bit_for_bit(name, N, lanes, B, terminal):
    s = solved(name, N, lanes, B, terminal)
    # the compact-writing prepare + the expand kernel against the dense prepare
    for k in FIELDS:
        assert torch.equal(s["nc"][k], s["nd"][k]), k
    assert torch.equal(s["ec"].t["reg"], s["ed"].t["reg"])
    # the compact fields are as wide as the library says (a zero-width field keeps one double)
    lib, fam = s["ec"]._lib, s["ec"].fam_c
    import ctypes
    for f, k in enumerate("ABQRM"):
        w = max(1, lib.noc_compact_width(ctypes.byref(fam), f))
        assert s["ec"].t[k].numel() == lib.noc_tiled_doubles(N, B, lanes, w)
    assert_same_result(s["rc"], s["rd"], s["ec"].tiled_blocks())


@pytest.mark.parametrize("terminal", [0, 1])
@pytest.mark.parametrize("B", [3, 37])
@pytest.mark.parametrize("name,N,lanes", CASES)
def test_compact_scan_matches_oracle(name, N, lanes, B, terminal):
    s = solved(name, N, lanes, B, terminal)
    rc, ref = s["rc"], s["ref"]
    for k in ("dx", "du", "pred"):
        e = relerr(getattr(rc, k).cpu().numpy(), ref[k])
        print(f"{name} N={N} L={lanes} B={B} terminal={terminal} {k}: rel err {e:.3e}")
        assert e < RTOL, k
    assert np.array_equal(rc.feasible.cpu().numpy().astype(bool), ref["feasible"].astype(bool))


@pytest.mark.parametrize("want_gains", [False, True])
def test_compact_scan_active_mask_x0_and_out(want_gains):
    """active with zeros in it (masked trajectories keep what `out` held), x0 set, out= reuse and
    want_gains=False, against the dense path and the oracle."""
    from noc import lqt
    name, N, lanes, B = "cartpole", 20, 8, 37
    s = solved(name, N, lanes, B, 0)
    ec, ed, nd = s["ec"], s["ed"], s["nd"]
    active = torch.ones(B, dtype=torch.int32, device="cuda")
    active[[0, 5, 6, 7, 8, 9, 10, 11, 36]] = 0  # a whole wave's segments (L = 8: 8 per wave) and stragglers
    x0 = torch.as_tensor(np.random.default_rng(5).normal(size=(B, 4)) * 0.1, device="cuda")
    dense = lqt.to_tiled(*(nd[k] for k in FIELDS), lanes)
    outs = []
    for tb, eng in ((ec.tiled_blocks(), ec), (dense, ed)):
        out = lqt.kkt_solve_tiled(tb, reg=eng.t["reg"], want_gains=want_gains)  # allocates
        for t in out:
            if t is not None:
                t.fill_(7)
        res = lqt.kkt_solve_tiled(tb, reg=eng.t["reg"], x0=x0, active=active, out=out)
        assert res is out
        outs.append(res)
    torch.cuda.synchronize()
    assert (outs[0].K is None) == (not want_gains)
    assert_same_result(outs[0], outs[1], dense, gains=want_gains)
    off = (active == 0).cpu().numpy()
    assert np.all(outs[0].dx.cpu().numpy()[off] == 7) and np.all(outs[0].pred.cpu().numpy()[off] == 7)
    case = dict(s["case"], x0=x0.cpu().numpy())
    case = {k: v[~off] for k, v in case.items()}
    ref = oracle_batch(case)
    for k in ("dx", "du", "pred"):
        assert relerr(getattr(outs[0], k).cpu().numpy()[~off], ref[k]) < RTOL, k
    assert np.array_equal(outs[0].feasible.cpu().numpy()[~off].astype(bool), ref["feasible"].astype(bool))


def test_compact_scan_two_waves_per_simd_instance():
    """B * lanes / 64 waves exceed the SIMDs: the launcher takes the 256-register instance (two
    waves per SIMD) that the c3 bench launch runs; N = 13 at 32 lanes also leaves 19 lanes empty."""
    from noc import lqt
    name, N, lanes, B = "cartpole", 13, 32, 2100
    simds = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    assert B * lanes // 64 > simds
    ec, ed = engines(name, N, lanes, B, 0)
    nd = ed.natural_blocks()
    for k, v in ec.natural_blocks().items():
        assert torch.equal(v, nd[k]), k
    rc = lqt.kkt_solve_tiled(ec.tiled_blocks(), reg=ec.t["reg"], want_gains=True)
    rd = lqt.kkt_solve_tiled(lqt.to_tiled(*(nd[k] for k in FIELDS), lanes), reg=ed.t["reg"],
                             want_gains=True)
    torch.cuda.synchronize()
    assert_same_result(rc, rd, ec.tiled_blocks())
    sample = list(range(0, B, B // 8))[:8]
    case = {k: nd[k][sample].cpu().numpy() for k in FIELDS}
    case["reg"] = ed.t["reg"][sample].cpu().numpy()
    ref = oracle_batch(case)
    for k in ("dx", "du", "pred"):
        assert relerr(getattr(rc, k)[sample].cpu().numpy(), ref[k]) < RTOL, k
    assert np.array_equal(rc.feasible[sample].cpu().numpy().astype(bool), ref["feasible"].astype(bool))


@pytest.mark.parametrize("mode", [0, 1])  # NOC_MODE_PAR, NOC_MODE_SEQ
@pytest.mark.parametrize("name,N,B", [("cartpole", 20, 5), ("pendulum", 20, 4)])
def test_launch_per_phase_loop_on_compact_blocks(name, N, B, mode):
    """The whole barrier schedule through noc_ipm_step*_compact against the dense loop."""
    from noc import problems
    from noc.ipm import BatchedIPM
    ocp = problems.make_problem(name, N)
    x0, u0 = problems.initial_conditions(name, N, B, seed=2)
    res = []
    for compact in (True, False):
        eng = BatchedIPM(ocp.family, N, B, compact=compact)
        eng.load(u0, x0)
        eng.solve(mode=mode)
        torch.cuda.synchronize()
        res.append(eng.result())
    for a, b, k in zip(res[0], res[1], ("u", "total_it", "kkt_solves")):
        assert torch.equal(a, b), k
    assert int(res[0][2].min()) > 0


def test_bench_blocks_fallbacks():
    """make_bench_blocks where the compact scan does not apply: the linear family (group solve)
    and two-wave segments (lanes = 128: the dense blocks expanded from the compact engine)."""
    from noc import lqt
    from noc.problems import make_bench_blocks
    cases = [("linear8", 16, 16, 0), ("cartpole", 20, 37, 0), ("cartpole", 20, 37, 128)]
    for name, N, B, lanes in cases:
        blocks = make_bench_blocks(name, N=N, batch=B, seed=1, lanes=lanes, natural=True)
        tb = blocks["tiled"]
        compact = name != "linear8" and tb.lanes <= 64
        assert isinstance(tb, lqt.CompactBlocks if compact else lqt.TiledBlocks), (name, tb.lanes)
        assert blocks["engine"].compact is (name != "linear8")
        if lanes:
            assert tb.lanes == lanes
        res = lqt.kkt_solve_tiled(tb, reg=blocks["reg"], want_gains=False)
        torch.cuda.synchronize()
        sample = [0, B // 2, B - 1]
        case = {k: blocks[k][sample].cpu().numpy() for k in FIELDS + ("reg",)}
        ref = oracle_batch(case)
        for k in ("dx", "du", "pred"):
            assert relerr(getattr(res, k)[sample].cpu().numpy(), ref[k]) < RTOL, (name, lanes, k)
        assert np.array_equal(res.feasible[sample].cpu().numpy().astype(bool),
                              ref["feasible"].astype(bool))
