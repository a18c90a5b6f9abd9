"""GPU checks of the compact KKT scan's chunk buffer (kkt_scan_impl.h: KEEP): the
compact A, B records of a chunk's first KEEP slots stay in registers from phase 3 to phase 4, the
slots past them are re-read, the first of those before the forward scan.

Everything goes through lqt.kkt_solve_tiled on compact blocks and is compared with the dense scan
on the expanded blocks by torch.equal (dx, du, pred, feasible, K, d: the buffer holds the records
phase 3 loaded and phase 4 expands them as the re-read would, so every double is the same) and with
oracle/noc_oracle.kkt_solve at RTOL = 1e-10, the tolerance of tests/test_scan_struct_gpu.py.

KEEP is read from the library (noc_kkt_compact_keep), so the boundary shapes follow the build.
Shapes, cart-pole and pendulum at lanes 8 and 32, batch 3 (an odd batch; at lanes 8 a wave shared
by trajectories and half empty, at lanes 32 two trajectories in one wave and a half-empty second):
N = lanes (KEEP - 1): the buffer's last slot is the chunk's last; N = lanes KEEP: every chunk fills
the buffer exactly; N = lanes KEEP + 3: three lanes re-read one slot past the buffer, the others
none; N = lanes - 1: a lane with no stage; N = lanes: one stage per lane, the hand-off alone.
Batch 3 at lanes 32 is routed to the one-wave-per-SIMD (512-register) cart-pole instance, as in
tests/test_scan_struct_gpu.py; the two-waves-per-SIMD (256-register) instance the bench line runs
takes batches whose waves outnumber the SIMDs, so one cart-pole case runs a batch of 2051 across
the buffer's boundary (oracle on its first two and its last trajectory).  One case masks a
trajectory; one runs backward then forward mode (dense natural blocks: forward mode has no phase 3
to fill a buffer and re-reads every slot)."""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from lq_cases import oracle_batch  # noqa: E402

pytestmark = pytest.mark.gpu
RTOL = 1e-10
FIELDS = ("A", "B", "Q", "R", "M", "r", "P")
B = 3
B_TWO_WAVES = 2051  # 1026 waves at lanes 32: more than one per SIMD, so not the 512-register instance
FAMILIES = ("cartpole", "pendulum")
LANES = (8, 32)
SHAPES = ("last_kept", "first_reread", "uneven", "empty_lane", "one_stage")


def relerr(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(1.0, float(np.max(np.abs(b)))))


@functools.lru_cache(maxsize=None)
def keep(name, lanes):
    from noc import problems, _lib
    lib = _lib.load()
    fam = problems.make_problem(name, 4).family.to_c()
    k = int(lib.noc_kkt_compact_keep(ctypes.byref(fam), lanes))
    assert k >= 1, (name, lanes, k)
    return k


def horizon(name, lanes, shape):
    k = keep(name, lanes)
    return {"last_kept": lanes * (k - 1), "first_reread": lanes * k, "uneven": lanes * k + 3,
            "empty_lane": lanes - 1, "one_stage": lanes}[shape]


@functools.lru_cache(maxsize=None)
def solved(name, N, lanes, batch=B, oracle_rows=None):
    """One case, computed once and shared (never modified): both engines' blocks, the compact and
    the dense fused solve (with gains, x0 set) and the oracle's solve of the dense blocks (of the
    trajectories `oracle_rows`, default all)."""
    from noc import lqt, problems, _lib
    from noc.ipm import BatchedIPM
    ocp = problems.make_problem(name, N)
    x0s, u0 = problems.initial_conditions(name, N, batch, seed=11)
    eng = {}
    for compact in (True, False):
        e = BatchedIPM(ocp.family, N, batch, lanes=lanes, compact=compact)
        assert e.compact is compact
        e.load(u0, x0s)
        e.init(0.1)
        e.prepare(_lib.MODE_PAR, 0)
        eng[compact] = e
    ec, ed = eng[True], eng[False]
    nd = ed.natural_blocks()
    nx = nd["A"].shape[-1]
    x0 = torch.as_tensor(np.random.default_rng(13).normal(size=(batch, nx)) * 0.1, device="cuda")
    tc = ec.tiled_blocks()
    td = lqt.to_tiled(*(nd[k] for k in FIELDS), lanes)
    assert isinstance(tc, lqt.CompactBlocks) and tc.lanes == lanes
    rc = lqt.kkt_solve_tiled(tc, reg=ec.t["reg"], x0=x0, want_gains=True)
    rd = lqt.kkt_solve_tiled(td, reg=ed.t["reg"], x0=x0, want_gains=True)
    torch.cuda.synchronize()
    rows = list(range(batch)) if oracle_rows is None else list(oracle_rows)
    case = {k: nd[k][rows].cpu().numpy() for k in FIELDS}
    case["reg"] = ed.t["reg"][rows].cpu().numpy()
    case["x0"] = x0[rows].cpu().numpy()
    return dict(ec=ec, ed=ed, nd=nd, tc=tc, td=td, x0=x0, rc=rc, rd=rd, rows=rows,
                ref=oracle_batch(case))


def assert_same_result(rc, rd, tb):
    from noc import lqt
    for k in ("dx", "du", "pred", "feasible"):
        assert torch.equal(getattr(rc, k), getattr(rd, k)), k
    for k, shape in (("K", (tb.Bt, tb.N, tb.nu, tb.nx)), ("d", (tb.Bt, tb.N, tb.nu))):
        assert torch.equal(lqt.untile(getattr(rc, k), shape, tb.lanes),
                           lqt.untile(getattr(rd, k), shape, tb.lanes)), k


def assert_matches_oracle(s, tag, res, rows=None):
    ref = s["ref"]
    rows = s["rows"] if rows is None else rows
    pick = [s["rows"].index(r) for r in rows]
    for k in ("dx", "du", "pred"):
        e = relerr(getattr(res, k)[rows].cpu().numpy(), ref[k][pick])
        print(f"{tag} {k}: rel err {e:.3e}")
        assert e < RTOL, (tag, k)
    assert np.array_equal(res.feasible[rows].cpu().numpy().astype(bool),
                          ref["feasible"][pick].astype(bool))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("name", FAMILIES)
def test_compact_equals_dense_and_oracle(name, lanes, shape):
    N = horizon(name, lanes, shape)
    s = solved(name, N, lanes)
    assert_same_result(s["rc"], s["rd"], s["td"])
    for tag, res in (("compact", s["rc"]), ("dense", s["rd"])):
        assert_matches_oracle(s, f"{name} N={N} L={lanes} {tag}", res)


def test_two_waves_per_simd_instance_across_the_boundary():
    """The 256-register cart-pole lanes-32 instance (the bench line's): a batch whose waves
    outnumber the SIMDs, chunks of KEEP and KEEP + 1 stages."""
    N = horizon("cartpole", 32, "uneven")
    rows = (0, 1, B_TWO_WAVES - 1)
    s = solved("cartpole", N, 32, batch=B_TWO_WAVES, oracle_rows=rows)
    assert_same_result(s["rc"], s["rd"], s["td"])
    assert_matches_oracle(s, f"cartpole N={N} L=32 B={B_TWO_WAVES} compact", s["rc"])


@pytest.mark.parametrize("name,lanes", [("cartpole", 8), ("pendulum", 32)])
def test_active_mask_kills_one_trajectory_of_a_wave(name, lanes):
    """Trajectory 1 of the three is masked off: it keeps what `out` held, the others are the
    compact = dense = oracle results, with chunks on both sides of the buffer's boundary."""
    from noc import lqt
    s = solved(name, horizon(name, lanes, "uneven"), lanes)
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
    for res in outs:
        assert bool((res.dx[1] == 7).all()) and bool((res.du[1] == 7).all())
        assert float(res.pred[1]) == 7 and int(res.feasible[1]) == 7
        assert_matches_oracle(s, f"{name} masked", res, rows=[0, 2])


def test_forward_mode_rereads_every_slot():
    """MODE_BWD then MODE_FWD on the natural blocks of the uneven cart-pole case: the forward pass
    composes and propagates from re-read A, B alone and gives the fused solve's step."""
    from noc import lqt
    lanes = 8
    s = solved("cartpole", horizon("cartpole", lanes, "uneven"), lanes)
    nd, ref = s["nd"], s["ref"]
    K, d, _, _, pred, feas = lqt.bwd_pass(*(nd[k] for k in FIELDS), reg=s["ed"].t["reg"], lanes=lanes)
    du, dx = lqt.fwd_pass(nd["A"], nd["B"], K, d, x0=s["x0"], lanes=lanes)
    torch.cuda.synchronize()
    for k, t in (("K", K), ("d", d), ("pred", pred), ("du", du), ("dx", dx)):
        e = relerr(t.cpu().numpy(), ref[k])
        print(f"bwd+fwd {k}: rel err {e:.3e}")
        assert e < RTOL, k
    assert np.array_equal(feas.cpu().numpy().astype(bool), ref["feasible"].astype(bool))
