"""The launch-per-phase trial kernel (csrc/ipm_kernels.hip: trial_kernel, through noc_ipm_trial
and noc_ipm_trial_params) on planted workspace states, against the accept step restated from the
reference (tests/accept_cases.py; its own preconditions: tests/test_accept_cases.py), and the
Newton iteration cap (P:201) in all three drivers.

The trial points are planted so that their total cost is exactly 0, 1 or inf in any summation
order (accept_cases.py: the planted table); the first assertion of every launch is that
noc_total_cost returns exactly that.  The gain is then two IEEE operations on planted doubles, and
everything the kernel writes must equal the restatement bit for bit (floats are compared as
their 64-bit patterns, so NaN and -0 count)."""
import ctypes
import dataclasses

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import accept_cases as AC

pytestmark = pytest.mark.gpu

REG_SENTINEL, REP_SENTINEL, ACTIVE_SENTINEL = -7.5, 5, 9
INT_FIELDS = ("it", "inner", "total_it", "kkt_solves")
F64_FIELDS = ("bp", "rp", "rinc", "cost", "hu", "gnorm")


def _family(kind):
    """A descriptor of the kind's kernel instance with goal 0, wx_0 = wf_0 = 2 and u_bound = 1:
    the kind and shape select the instance, the numbers make the planted costs exact."""
    from noc import problems
    if kind == "pendulum":
        fam = problems.pendulum(0.05).family
    elif kind == "cartpole":
        fam = problems.cartpole(0.05).family
    elif kind == "linear8":
        fam = problems.double_integrators(4, 0.001, constrained=True).family
    else:
        import custom_families as CF
        fam = CF.actuated_pendulum(1.0 / 50).family
    nx, nu = fam.nx, fam.nu
    return dataclasses.replace(fam, goal=[0.0] * nx, wx=[2.0] + [1.0] * (nx - 1), wu=[1.0] * nu,
                               wf=[2.0] + [1.0] * (nx - 1), u_bound=1.0)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _plant(eng, rows):
    """Write the rows into the engine's workspace; returns the host copies (x, dx, u, du)."""
    Bt, N, nx, nu = eng.Bt, eng.N, eng.nx, eng.nu
    assert len(rows) == Bt
    k_, i_ = np.meshgrid(np.arange(N + 1), np.arange(nx), indexing="ij")
    x = np.broadcast_to(0.5 + 0.25 * ((k_ + i_) % 3), (Bt, N + 1, nx)).copy()
    k_, j_ = np.meshgrid(np.arange(N), np.arange(nu), indexing="ij")
    u = np.broadcast_to(0.125 * (1 + j_) + 0.0 * k_, (Bt, N, nu)).copy()
    dx, du = -x, -u                                  # x + dx = +0, u + du = +0, exactly
    for b, r in enumerate(rows):
        at = r.get("at", min(2, N - 1))
        if r["trial"] == "one":                      # e_0 = 3 - 2 = 1 at one stage (or at x_N)
            x[b, at, 0], dx[b, at, 0] = 3.0, -2.0
        elif r["trial"] == "infeasible":             # one control at 0.5 + 1.5 = 2 > u_bound
            u[b, at, nu - 1], du[b, at, nu - 1] = 0.5, 1.5
    t = eng.t
    for name, arr in (("x", x), ("dx", dx), ("u", u), ("du", du)):
        t[name].copy_(torch.as_tensor(arr))
    col = lambda k: np.array([r["state"][k] for r in rows])
    for k in F64_FIELDS:
        t[k].copy_(torch.as_tensor(col(k).astype(np.float64)))
    for k in INT_FIELDS:
        t[k].copy_(torch.as_tensor(col(k).astype(np.int32)))
    t["pred"].copy_(torch.as_tensor(np.array([r["pred"] for r in rows], np.float64)))
    t["feasible"].copy_(torch.as_tensor(np.array([r["feasible"] for r in rows], np.int32)))
    t["phase"].copy_(torch.as_tensor(np.array([r["phase"] for r in rows], np.int32)))
    t["reg"].fill_(REG_SENTINEL)
    t["repeats"].fill_(REP_SENTINEL)
    t["kkt_active"].fill_(ACTIVE_SENTINEL)
    return x, dx, u, du


def _check_planted_cost(eng, rows, x, dx, u, du, ubound=None):
    """noc_total_cost / noc_check_feasibility at the planted trial points: exactly 0 or 1, and
    infeasible exactly where planted."""
    from noc import _lib
    dev = eng.device
    xt = torch.as_tensor(x + dx, device=dev).contiguous()
    ut = torch.as_tensor(u + du, device=dev).contiguous()
    cost = torch.full((eng.Bt,), -3.0, device=dev, dtype=torch.float64)
    ok = torch.full((eng.Bt,), -3, device=dev, dtype=torch.int32)
    fam = ctypes.byref(eng.fam_c)
    s = eng._stream()
    _lib.check(eng._lib.noc_total_cost(fam, eng.N, eng.Bt, xt.data_ptr(), ut.data_ptr(),
                                       eng.t["bp"].data_ptr(), cost.data_ptr(), s), "noc_total_cost",
               eng._lib)
    _lib.check(eng._lib.noc_check_feasibility(fam, eng.N, eng.Bt, xt.data_ptr(), ut.data_ptr(),
                                              ok.data_ptr(), s), "noc_check_feasibility", eng._lib)
    cost, ok = cost.cpu().numpy(), ok.cpu().numpy()
    for b, r in enumerate(rows):
        want = AC.trial_cost(r["trial"])
        assert ok[b] == (0 if want == AC.INF else 1), (r["name"], ok[b])
        if want != AC.INF:
            assert cost[b] == want and not np.signbit(cost[b]), (r["name"], cost[b])


def _launch_and_compare(eng, rows, mode, flags, with_repeats, params=None, costs=None):
    from noc import _lib
    x, dx, u, du = _plant(eng, rows)
    if params is None:
        _check_planted_cost(eng, rows, x, dx, u, du)
    eng.ws.flags = flags
    eng.ws.repeats = eng.t["repeats"].data_ptr() if with_repeats else None
    m = _lib.MODE_PAR if mode == AC.PAR else _lib.MODE_SEQ
    fam, ws = ctypes.byref(eng.fam_c), ctypes.byref(eng.ws)
    if params is None:
        _lib.check(eng._lib.noc_ipm_trial(fam, ws, m, eng._stream()), "noc_ipm_trial", eng._lib)
    else:
        _lib.check(eng._lib.noc_ipm_trial_params(fam, ws, params.data_ptr(), m, eng._stream()),
                   "noc_ipm_trial_params", eng._lib)
    torch.cuda.synchronize()
    got = {k: eng.t[k].cpu().numpy() for k in F64_FIELDS + INT_FIELDS
           + ("phase", "reg", "repeats", "kkt_active", "x", "u", "pred", "feasible")}
    for b, r in enumerate(rows):
        tag = (r["name"], "par" if mode == AC.PAR else "seq", flags, with_repeats)
        if r["phase"] != AC.SOLVE:
            st, o = dict(r["state"]), None
        else:
            new_cost = AC.trial_cost(r["trial"]) if costs is None else costs[b]
            st, o = AC.accept_step(r["state"], mode, new_cost, r["pred"], r["feasible"] != 0, flags)
        phase = r["phase"] if o is None else o["phase"]
        if phase == AC.ROLLOUT and o is not None:
            phase = AC.ROLLOUT_PENDING              # the next step's rollout picks it up
        assert got["phase"][b] == phase, (tag, got["phase"][b], phase, o)
        for k in INT_FIELDS:
            assert got[k][b] == st[k], (tag, k, got[k][b], st[k])
        for k in F64_FIELDS:                        # cost, hu, gnorm: untouched (st carries them)
            assert _bits(got[k][b:b + 1])[0] == _bits(np.array([float(st[k])]))[0], \
                (tag, k, got[k][b], st[k])
        reg = REG_SENTINEL if o is None or o["reg"] is None else o["reg"]
        assert _bits(got["reg"][b:b + 1])[0] == _bits(np.array([float(reg)]))[0], (tag, got["reg"][b], reg)
        rep = o["rep"] if (o is not None and with_repeats) else 0
        assert got["repeats"][b] == REP_SENTINEL + rep, (tag, got["repeats"][b], rep)
        assert got["kkt_active"][b] == ACTIVE_SENTINEL, tag
        take = o is not None and o["take"]
        wx, wu = (x[b] + dx[b], u[b] + du[b]) if take else (x[b], u[b])   # one add per entry
        assert np.array_equal(_bits(got["x"][b]), _bits(wx)), (tag, "x", take)
        assert np.array_equal(_bits(got["u"][b]), _bits(wu)), (tag, "u", take)
        assert _bits(got["pred"][b:b + 1])[0] == _bits(np.array([float(r["pred"])]))[0], tag
        assert got["feasible"][b] == r["feasible"], tag


_ENGINES = {}


def _engine(kind, N, Bt):
    from noc.ipm import BatchedIPM
    key = (kind, N, Bt)
    if key not in _ENGINES:
        _ENGINES[key] = BatchedIPM(_family(kind), N, Bt, persistent=False, compact=False)
    return _ENGINES[key]


@pytest.mark.parametrize("kind,N", [("pendulum", 5), ("cartpole", 7), ("linear8", 3),
                                    ("actuated_pendulum", 6)])
@pytest.mark.parametrize("mode", [AC.PAR, AC.SEQ], ids=["par", "seq"])
def test_trial_kernel_decisions_on_planted_states(kind, N, mode):
    """The whole planted table, one batch row per case, one launch per flag set and with
    ws.repeats set and NULL: phase, counters, rp, r_inc, bp, reg, the repeats accounted and x, u
    equal the restatement bit for bit; cost, hu, gnorm, pred, feasible and kkt_active, and every
    field of a row that is not at SOLVE, keep their planted values."""
    rows = AC.planted_rows()
    assert len(rows) % 4 != 0
    eng = _engine(kind, N, len(rows))
    for flags in (0, AC.ONE_STAGE, AC.NO_REPEAT_SKIP):
        for with_repeats in (True, False):
            _launch_and_compare(eng, rows, mode, flags, with_repeats)


def _coverage_rows(N, trial):
    """Row k: the only non-zero stage cost (or the only infeasible control) at stage k; the last
    row: in the final cost (or no infeasible control at all).  cost 1.5, pred -1: a feasible
    trial of cost 1 gives gain 0.5 (shrink 1), one whose stage was dropped gain 1.5 (shrink 1/3);
    an infeasible one is rejected, one whose vote was dropped accepted."""
    rows = []
    for k in range(N + 1):
        r = AC._row(f"{trial}_at_{k}", "x", cost=1.5, rp=0.75, inner=0)
        r["trial"], r["at"] = trial, k
        if trial == "infeasible" and k == N:
            r["trial"] = "zero"
        rows.append(r)
    return rows


@pytest.mark.parametrize("N", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("trial", ["one", "infeasible"])
def test_trial_sum_and_feasibility_vote_see_every_stage(N, trial):
    """Horizons with a lane without a stage (N = 1, 63), exactly one stage per lane, and lanes
    with two and three stages: a dropped stage, a dropped vote or an update loop that misses a
    stage (k <= N) changes rp or x of that row."""
    rows = _coverage_rows(N, trial)
    eng = _engine("pendulum", N, N + 1)
    for mode in (AC.PAR, AC.SEQ):
        _launch_and_compare(eng, rows, mode, 0, True)
    for b, r in enumerate(rows):                    # the rows do tell the two outcomes apart
        _, o = AC.accept_step(r["state"], AC.PAR, AC.trial_cost(r["trial"]), -1.0, True)
        _, dropped = AC.accept_step(r["state"], AC.PAR, 0.0, -1.0, True)
        assert (o["gain"], o["take"]) != (dropped["gain"], dropped["take"]) or r["trial"] == "zero"


@pytest.mark.parametrize("kind,N", [("pendulum", 5), ("linear8", 3)])
def test_trial_params_kernel_uses_each_trajectorys_own_bound(kind, N):
    """noc_ipm_trial_params: one control of every trial at u + du = 2.  The family's bound is 1
    (infeasible) or 4 (feasible); a row's own record says 4 or 1 the other way round, or repeats
    the family's.  With bp = 0 and the record's wu = 0 the feasible trial's cost is exactly 0 (the
    barrier term is multiplied by bp = 0), so the decisions stay bit-exact."""
    from noc.ipm import BatchedIPM
    from noc.traj_params import TrajectoryParams, pack
    base = AC.planted_rows()
    pick = [r for r in base if r["name"] in ("gain_half", "gain_negative", "gain_fused2",
                                             "bwd_infeasible", "cap_inner_to_501", "clip_hi_inner250",
                                             "phase_done")]
    for fam_bound, own in ((1.0, (4.0, 1.0)), (4.0, (1.0, 4.0))):
        rows, bounds = [], []
        for r in pick:
            for ub in own:
                r2 = dict(r, state=dict(r["state"], bp=0.0), trial="infeasible",
                          name=f"{r['name']}_ub{ub}")
                rows.append(r2)
                bounds.append(ub)
        assert len(rows) % 4 != 0
        fam = dataclasses.replace(_family(kind), u_bound=fam_bound)
        eng = BatchedIPM(fam, N, len(rows), persistent=False, compact=False)
        rec = pack(TrajectoryParams(u_bound=np.array(bounds), wu=np.zeros(fam.nu)), fam, len(rows))
        params = torch.as_tensor(rec, device=eng.device).contiguous()
        costs = [AC.INF if ub < 2.0 else 0.0 for ub in bounds]
        assert AC.INF in costs and 0.0 in costs
        for mode in (AC.PAR, AC.SEQ):
            _launch_and_compare(eng, rows, mode, 0, True, params=params, costs=costs)


# ------------------------------------------------------------------------------------------------
_KEYS = ("total_it", "kkt_solves", "phase", "it", "inner")


@pytest.mark.parametrize("N", [20, 130])
def test_newton_iteration_cap_ends_the_stage_in_every_driver(N, monkeypatch):
    """P:201: a barrier stage ends once iteration_counter > 1000.  A pendulum batch is taken to
    mid-stage by the launch-per-phase driver, `it` is overwritten with 1000 on every trajectory
    still running, and the stage (NOC_WS_ONE_STAGE) is continued by the launch-per-phase loop, by
    the one-wave kernel and by the wide kernel (NOC_WS_RESUME): each ends it after exactly one
    more Newton iteration, total_it = 1001, with identical counters."""
    from noc import problems, _lib
    from noc.ipm import BatchedIPM
    Bt = 4
    ocp = problems.make_problem("pendulum", N)
    x0, u0 = problems.initial_conditions("pendulum", N, Bt, seed=33)
    mode, term = _lib.MODE_PAR, _lib.TERMINAL_STAGE0
    base = BatchedIPM(ocp.family, N, Bt, lanes=64, persistent=False, overlap=False)
    base.ws.flags = _lib.WS_ONE_STAGE
    base.load(u0, x0)
    base.init(0.1)
    for _ in range(3):
        base.step(mode, term)
    torch.cuda.synchronize()
    running = base.t["phase"] != _lib.PHASE_DONE
    assert bool(running.all()) and int(base.t["total_it"].max()) == 0      # mid-stage, stage one
    assert int(base.t["it"].max()) < 1000
    base.t["it"][running] = 1000
    snap = {k: base.t[k].clone() for k in BatchedIPM._SHARED_FIELDS}
    out = {}
    for driver, wide in (("one_wave", "0"), ("wide", "1")):
        monkeypatch.setenv("NOC_PERSIST_WIDE", wide)
        eng = BatchedIPM(ocp.family, N, Bt, lanes=64, persistent=True)
        for k, v in snap.items():
            eng.t[k].copy_(v)
        eng.ws.flags = _lib.WS_ONE_STAGE
        eng.solve_persistent(mode=mode, resume=True, schedule="index")
        torch.cuda.synchronize()
        out[driver] = {k: eng.t[k].cpu().numpy().copy() for k in _KEYS + ("u", "bp")}
    for _ in range(80):                                # <= 501 accounted retries per step
        for _ in range(8):
            base.step(mode, term)
        if base.all_done():
            break
    torch.cuda.synchronize()
    out["loop"] = {k: base.t[k].cpu().numpy().copy() for k in _KEYS + ("u", "bp")}
    for driver, o in out.items():
        assert np.all(o["phase"] == _lib.PHASE_DONE), (driver, o["phase"])
        assert np.all(o["total_it"] >= 1001), (driver, o["total_it"])      # the cap did fire
        assert np.all(o["total_it"] == 1001), (driver, o["total_it"])      # one more iteration
        assert np.all(o["bp"] == 0.1 / 5), (driver, o["bp"])
        for k in _KEYS:
            assert np.array_equal(o[k], out["loop"][k]), (driver, k, o[k], out["loop"][k])
    scale = max(1.0, float(np.max(np.abs(out["loop"]["u"]))))
    assert np.max(np.abs(out["one_wave"]["u"] - out["loop"]["u"])) <= 1e-12 * scale
    assert np.max(np.abs(out["wide"]["u"] - out["loop"]["u"])) <= 1e-8 * scale
