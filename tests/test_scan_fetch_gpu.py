"""GPU checks of the scans' folded partner fetches (csrc/small_linalg.h: sklansky_fetch_select;
kkt_scan_impl.h: FOLD): in the stand-alone nx = 4 scan kernels at two waves per
SIMD (256 registers) every level 0-4 of the reverse and of the forward Sklansky scan fetches a
partner's dword and selects it against the identity element's in ONE instruction (v_cndmask_b32
with a DPP source, VCC = the lanes that do not combine at the level) instead of a DPP move and a
select.  Moves and selects only, so every double of every result is what it was: the compact scan
must still equal the dense scan on the expanded blocks by torch.equal (dx, du, pred, feasible, K,
d), and both the oracle (oracle/noc_oracle.kkt_solve) at RTOL = 1e-10, the tolerance of
tests/test_scan_struct_gpu.py and tests/test_scan_keep_gpu.py, whose helpers this file uses.

Shapes.  Cart-pole at lanes 8, 16, 32 and 64: a segment of L lanes runs the fetch levels
0 .. log2(L) - 1, the last of them value-only, so the four widths together run every level 0-5 in
both forms (level 5, a v_readlane, is not folded and must still agree).  N = lanes - 1 (a lane
with no stage: its element is the identity going in), N = lanes (one stage per lane) and
N = 2 lanes + 3 (chunks of two and three stages).  Batch 3 is an odd batch (a wave shared by
trajectories and partly empty at lanes < 64); at lanes 32 and 64 its waves fit one per SIMD and
the launch takes the 512-register instance, whose combines are masked and fetch without selects,
so those two widths also run a batch of 2051 -- more waves than SIMDs, the 256-register instance
with the folded fetches, as tests/test_scan_keep_gpu.py chooses it (oracle on its first two and
its last trajectory).  Lanes 8 and 16 have only the 256-register instance.  Pendulum (nx = 2:
masked at every width, nothing folded) at lanes 8 and 64 guards the shared code.

One case masks a trajectory of a shared wave; one runs backward then forward mode (the forward
scan alone, from stored gains).  The pivoting cases take the rand_lq batches of
tests/neighbour_cases.py through the helpers of tests/test_kkt_neighbours_gpu.py: a wave in which
exactly ONE trajectory's elimination check fails (by the CPU model of the pivot decision, with
margins on both sides of the device's threshold), so the whole wave redoes the level with the
pivoting solve after re-fetching; its wave-mates, copies of one clean trajectory, must equal that
trajectory solved alone bit for bit, in the 256-register instances of lanes 8, 16 and 32."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import neighbour_cases as NC  # noqa: E402
import test_kkt_neighbours_gpu as NG  # noqa: E402  (helpers only: _case, _rows, _solve, _same, _accurate)
import test_scan_keep_gpu as SK  # noqa: E402  (helpers only: solved, assert_same_result, assert_matches_oracle)

pytestmark = pytest.mark.gpu
RTOL = SK.RTOL  # 1e-10
B = 3
B_TWO_WAVES = SK.B_TWO_WAVES  # 2051: more waves than SIMDs at lanes 32 and at lanes 64
LANES = (8, 16, 32, 64)
SHAPES = ("empty_lane", "one_stage", "uneven")


def horizon(lanes, shape):
    return {"empty_lane": lanes - 1, "one_stage": lanes, "uneven": 2 * lanes + 3}[shape]


def check(s, tag):
    SK.assert_same_result(s["rc"], s["rd"], s["td"])
    for which, res in (("compact", s["rc"]), ("dense", s["rd"])):
        SK.assert_matches_oracle(s, f"{tag} {which}", res)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("lanes", LANES)
def test_cartpole_compact_equals_dense_and_oracle(lanes, shape):
    N = horizon(lanes, shape)
    check(SK.solved("cartpole", N, lanes), f"cartpole N={N} L={lanes} B={B}")


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("lanes", (32, 64))
def test_cartpole_two_waves_per_simd_instance(lanes, shape):
    """The 256-register instances of lanes 32 (the bench line's) and 64: the folded fetches."""
    N = horizon(lanes, shape)
    rows = (0, 1, B_TWO_WAVES - 1)
    s = SK.solved("cartpole", N, lanes, batch=B_TWO_WAVES, oracle_rows=rows)
    check(s, f"cartpole N={N} L={lanes} B={B_TWO_WAVES}")


@pytest.mark.parametrize("lanes", (8, 64))
def test_pendulum_compact_equals_dense_and_oracle(lanes):
    N = horizon(lanes, "uneven")
    check(SK.solved("pendulum", N, lanes), f"pendulum N={N} L={lanes} B={B}")


def test_active_mask_kills_one_trajectory_of_a_wave():
    """Trajectory 1 of the three (one wave at lanes 16) is masked off: it keeps what `out` held,
    the others are the compact = dense = oracle results."""
    from noc import lqt
    s = SK.solved("cartpole", horizon(16, "uneven"), 16)
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
    SK.assert_same_result(outs[0], outs[1], s["td"])
    for res in outs:
        assert bool((res.dx[1] == 7).all()) and bool((res.du[1] == 7).all())
        assert float(res.pred[1]) == 7 and int(res.feasible[1]) == 7
        SK.assert_matches_oracle(s, "cartpole masked", res, rows=[0, 2])


@pytest.mark.parametrize("lanes,batch", [(16, B), (32, B_TWO_WAVES)])
def test_backward_then_forward_mode(lanes, batch):
    """MODE_BWD then MODE_FWD on the natural blocks: the reverse scan alone, then the forward scan
    alone from the stored gains, against the oracle; the pair gives the fused solve's step."""
    from noc import lqt
    rows = None if batch == B else (0, 1, batch - 1)
    s = SK.solved("cartpole", horizon(lanes, "uneven"), lanes, batch=batch, oracle_rows=rows)
    nd, ref, pick = s["nd"], s["ref"], s["rows"]
    K, d, _, _, pred, feas = lqt.bwd_pass(*(nd[k] for k in SK.FIELDS), reg=s["ed"].t["reg"], lanes=lanes)
    du, dx = lqt.fwd_pass(nd["A"], nd["B"], K, d, x0=s["x0"], lanes=lanes)
    torch.cuda.synchronize()
    for k, t in (("K", K), ("d", d), ("pred", pred), ("du", du), ("dx", dx)):
        e = SK.relerr(t[pick].cpu().numpy(), ref[k])
        print(f"bwd+fwd L={lanes} B={batch} {k}: rel err {e:.3e}")
        assert e < RTOL, k
    assert np.array_equal(feas[pick].cpu().numpy().astype(bool), ref["feasible"].astype(bool))
    for k, t in (("dx", dx), ("du", du), ("pred", pred)):
        e = SK.relerr(t.cpu().numpy(), getattr(s["rd"], k).cpu().numpy())
        print(f"bwd+fwd L={lanes} B={batch} {k} vs fused: rel err {e:.3e}")
        assert e < RTOL, k


# (case of neighbour_cases.CASES, rows of the batch as a function of (failing f, clean mate m)):
# one failing trajectory among copies of a clean wave-mate, all in the 256-register instance
PIVOT = [
    (NC.CASES[1], lambda f, m: [m] * 3 + [f] + [m] * 4),        # lanes 8: one full wave
    (NC.CASES[2], lambda f, m: [m, f, m, m]),                   # lanes 16: one full wave
    (NC.CASES[4], lambda f, m: [f, m] + [m] * (B_TWO_WAVES - 2)),  # lanes 32: 1026 waves
]


@pytest.mark.parametrize("case,layout", PIVOT, ids=[NC.IDS[NC.CASES.index(c)] for c, _ in PIVOT])
def test_one_failing_check_redoes_the_wave_and_leaves_its_mates_alone(case, layout):
    nx, nu, N, lanes, _, _ = case
    assert nx == 4
    data, ref, dev = NG._case(case)
    failing, clean, witnesses = NC.classify(case, data)
    assert witnesses, "the case no longer mixes a failing and a clean trajectory in a wave"
    _, _, f, m = witnesses[0]
    assert f in failing and m in clean and m not in failing
    rows = layout(f, m)
    assert rows.count(f) == 1
    full = NG._solve(NG._rows(dev, rows), lanes, want_value=True)
    solo = NG._solve(NG._rows(dev, [m]), lanes, want_value=True)
    torch.cuda.synchronize()
    per = 64 // lanes
    mates = [i for i in range(per) if rows[i] == m]  # the failing trajectory's wave
    assert len(mates) == min(per, len(rows)) - 1 and rows.index(f) < per
    for i in mates:
        NG._same({k: v[i:i + 1] for k, v in full.items()}, solo, i)
    last = len(rows) - 1  # a copy in a wave without a failing trajectory (or the same wave)
    NG._same({k: v[last:last + 1] for k, v in full.items()}, solo, last)
    head = list(range(min(per, len(rows))))
    NG._accurate({k: v[head] for k, v in full.items()}, ref, rows=[rows[i] for i in head])
