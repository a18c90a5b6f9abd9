"""Per-trajectory cost parameters in interior-point DDP and the building blocks, host side (no
GPU): the additive C-ABI entry points exist and refuse bad arguments before any device call,
ddp_sharded hands every rank the rows of its shard, the nx > 4 building-block loop hands the record
to the blocks that read a cost parameter (and to no other), and the public calls refuse params on
unbatched inputs (NocError) and a params object of another type (ValueError)."""
import ctypes
import os

import numpy as np
import pytest
import torch.multiprocessing as mp

NEW_SYMBOLS = ["noc_ddp_params_supported", "noc_ddp_solve_params", "noc_derivatives_params",
               "noc_final_cost_derivs_params", "noc_check_feasibility_params",
               "noc_total_cost_params"]


def _lib_and_problems():
    from noc import _lib, problems
    return _lib, _lib.load(), problems


def test_symbols_exist_and_the_abi_version_is_unchanged():
    _lib, lib, _ = _lib_and_problems()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert lib.noc_abi_version() == 5


def test_ddp_params_supported_query():
    _, lib, problems = _lib_and_problems()
    sup = lambda fam: lib.noc_ddp_params_supported(ctypes.byref(fam))
    for ocp in (problems.pendulum(0.02), problems.cartpole(0.005), problems.double_integrators(1, 0.1)):
        assert sup(ocp.family.to_c()) == 1
    lin8 = problems.double_integrators(4, 0.001).family.to_c()
    assert (lin8.nx, lin8.nu) == (8, 4)
    assert sup(lin8) == 0                      # nx > 4: no one-launch kernel
    bad = problems.pendulum(0.02).family.to_c()
    bad.kind = 77
    assert sup(bad) == 0
    assert lib.noc_ddp_params_supported(None) == 0


P = 4096  # a fake, aligned, non-NULL device pointer: argument checks run before any device call


def _calls(lib, f, p, N=10, bp0=0.1):
    return {"ddp": lambda: lib.noc_ddp_solve_params(f, N, 2, P, P, P, P, P, P, p, bp0, 100, 0, None),
            "derivatives": lambda: lib.noc_derivatives_params(f, N, 2, *([P] * 13), p, None),
            "final": lambda: lib.noc_final_cost_derivs_params(f, 2, P, P, P, p, None),
            "feasibility": lambda: lib.noc_check_feasibility_params(f, N, 2, P, P, P, p, None),
            "total_cost": lambda: lib.noc_total_cost_params(f, N, 2, P, P, P, P, p, None)}


def _refused(lib, fn, word):
    assert fn() == -1
    assert word in lib.noc_last_error(), lib.noc_last_error()


def test_argument_errors_return_minus_one_with_a_message():
    _, lib, problems = _lib_and_problems()
    cart = problems.cartpole(0.005).family.to_c()
    fam = ctypes.byref(cart)
    for fn in _calls(lib, fam, None).values():                 # NULL params
        _refused(lib, fn, b"params is NULL")
    bad = problems.cartpole(0.005).family.to_c()
    bad.kind = 77
    for fn in _calls(lib, ctypes.byref(bad), P).values():      # an unsupported family
        _refused(lib, fn, b"unsupported family")
    lin8 = problems.double_integrators(4, 0.001).family.to_c()
    _refused(lib, _calls(lib, ctypes.byref(lin8), P)["ddp"], b"unsupported family")  # nx > 4
    for fn in _calls(lib, None, P).values():                   # NULL family
        _refused(lib, fn, b"family is NULL")
    for bp0 in (float("nan"), -0.1, float("inf")):             # the bp0 rule of noc_ddp_solve_ex
        _refused(lib, _calls(lib, fam, P, bp0=bp0)["ddp"], b"bp0")
    for name in ("ddp", "derivatives", "feasibility", "total_cost"):  # what the twins refuse
        _refused(lib, _calls(lib, fam, P, N=0)[name], b"N")
    assert lib.noc_ddp_solve_params(fam, 10, 2, P, P, P, P, P, P, P, 0.1, 0, 0, None) == -1
    assert b"max_passes" in lib.noc_last_error()
    assert lib.noc_ddp_solve_params(fam, 10, 2, P, P, P, P, P, P, P, 0.1, 100, 2, None) == -1
    assert b"flags" in lib.noc_last_error()
    assert lib.noc_ddp_solve_params(fam, 10, 2, None, P, P, P, P, P, P, 0.1, 100, 0, None) == -1
    assert b"x0" in lib.noc_last_error()
    assert lib.noc_total_cost_params(fam, 10, 2, P, P, P, P, P + 8, None) == -1
    assert b"aligned" in lib.noc_last_error()


# ------------------------------------------------------------------------------- ddp_sharded
def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _full_params(B):
    import noc
    from noc import problems
    fam = problems.pendulum(0.02).family
    b = np.arange(B, dtype=np.float64)
    goal = np.tile(np.asarray(fam.goal, dtype=np.float64), (B, 1))
    goal[:, 0] += 0.1 * b
    return fam, noc.TrajectoryParams(goal=goal, wu=[0.5], u_bound=2.0 + b)


def _shard_worker(rank, world, port, B, with_params, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from noc import distributed as D
    from noc.traj_params import pack
    fam, params = _full_params(B)
    seen = []

    def fake_with(ocp, u, x0, return_info=True, params=None):
        seen.append(None if params is None else pack(params, fam, u.shape[0]))
        b = np.round(x0[:, 0]).astype(int)
        return u + b[:, None, None], (10 + b).astype(np.int32), dict(
            passes=(20 + b).astype(np.int32), done=np.ones(len(b), dtype=bool))

    def fake_without(ocp, u, x0, return_info=True):  # a `params` keyword would be a TypeError
        seen.append("no keyword")
        return fake_with(ocp, u, x0)

    u = np.arange(B * 5, dtype=np.float64).reshape(B, 5, 1)
    x0 = np.zeros((B, 2))
    x0[:, 0] = np.arange(B)
    if with_params:
        U, it, passes = D.ddp_sharded(None, u, x0, ddp_fn=fake_with, params=params)
    else:
        U, it, passes = D.ddp_sharded(None, u, x0, ddp_fn=fake_without)
    q.put((rank, U, it, seen))
    dist.destroy_process_group()


def _run_world2(B, with_params):
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_shard_worker, args=(r, world, port, B, with_params, q))
             for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return {r[0]: r[1:] for r in res}


@pytest.mark.parametrize("B", [5, 1])
def test_ddp_sharded_hands_every_rank_the_rows_of_its_shard(B):
    """B = 1: rank 1 holds an empty shard and calls nothing."""
    from noc.distributed import shard_bounds
    from noc.traj_params import pack
    fam, params = _full_params(B)
    full = pack(params, fam, B)
    res = _run_world2(B, True)
    for rank, (U, it, seen) in res.items():
        lo, hi = shard_bounds(B, 2, rank)
        if hi == lo:
            assert seen == []
            continue
        assert len(seen) == 1 and seen[0] is not None
        assert np.array_equal(seen[0], full[lo:hi])
        assert np.array_equal(seen[0], pack(params.rows(lo, hi), fam, hi - lo))
        assert np.array_equal(it, 10 + np.arange(B))   # the gather is unchanged


def test_ddp_sharded_without_params_passes_no_keyword():
    res = _run_world2(3, False)
    for rank, (U, it, seen) in res.items():
        assert seen and seen[0] == "no keyword"


# ------------------------------------------------------------------- the building-block loop
def test_building_block_loop_hands_the_record_to_the_blocks_that_read_it(monkeypatch):
    """_solve_blocks with params on the CPU, its device blocks replaced by the oracle's (as
    test_building_block_loop_control_flow_on_cpu): total_cost, compute_derivatives,
    check_traj_feasibility and bwd_pass receive the very record on every call, nonlin_rollout
    receives no params keyword, and the loop's results do not depend on the hand-over itself."""
    import torch
    from noc import differential_dynamic_programming as D
    from noc.optimal_control_problem import Derivatives
    from oracle import noc_oracle as O, problems as PR
    N, Bt = 8, 2
    prob = O.NumpyProblem(PR.pendulum_ocp(1.0 / N))
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))
    npy = lambda a: a.detach().cpu().numpy()
    got = dict(total_cost=[], compute_derivatives=[], bwd_pass=[], check_traj_feasibility=[],
               nonlin_rollout=0)
    MISSING = object()

    def total_cost(ocp, x, u, bp, params=MISSING):
        got["total_cost"].append(params)
        return t([prob.total_cost(npy(x[b]), npy(u[b]), bp) for b in range(x.shape[0])])

    def compute_derivatives(ocp, x, u, bp, params=MISSING):
        got["compute_derivatives"].append(params)
        per = [prob.derivatives(npy(x[b]), npy(u[b]), bp) for b in range(x.shape[0])]
        return Derivatives(*(t(np.stack([p[i] for p in per])) for i in range(10)))

    def bwd_pass(ocp, xN, d, rp, params=MISSING):
        got["bwd_pass"].append(params)
        out = []
        for b in range(xN.shape[0]):
            Vx, Vxx = prob.final_grad_hess(npy(xN[b]))
            out.append(O.ddp_bwd_pass(Vx, Vxx, tuple(npy(f[b]) for f in d), float(rp[b])))
        k, K, pred, feas, Hu = zip(*out)
        return t(np.stack(k)), t(np.stack(K)), t(pred), torch.tensor(feas), t(np.stack(Hu))

    def nonlin_rollout(ocp, K, k, x, u):  # a params keyword here would be a TypeError
        got["nonlin_rollout"] += 1
        out = [O.ddp_nonlin_rollout(prob, npy(K[b]), npy(k[b]), npy(x[b]), npy(u[b]))
               for b in range(x.shape[0])]
        return t(np.stack([o[0] for o in out])), t(np.stack([o[1] for o in out]))

    def feasible(ocp, x, u, params=MISSING):
        got["check_traj_feasibility"].append(params)
        return torch.tensor([prob.feasible(npy(x[b]), npy(u[b])) for b in range(x.shape[0])])

    for name, fn in dict(total_cost=total_cost, compute_derivatives=compute_derivatives,
                         bwd_pass=bwd_pass, nonlin_rollout=nonlin_rollout,
                         check_traj_feasibility=feasible).items():
        monkeypatch.setattr(D, name, fn)
    rng = np.random.default_rng(17)
    x0 = np.array([0.1, -0.1]) + 0.01 * rng.normal(size=(Bt, 2))
    u0 = 0.1 * rng.normal(size=(Bt, N, 1))
    record = t(np.zeros((Bt, 32)))
    with_p = D._solve_blocks(None, t(u0), t(x0), 0.1, 6, 0, params=record)
    readers = ("total_cost", "compute_derivatives", "bwd_pass", "check_traj_feasibility")
    for name in readers:
        assert got[name] and all(p is record for p in got[name]), name
    assert got["nonlin_rollout"] > 0
    # params=None: every block is called exactly as before (no keyword at all)
    for name in readers:
        got[name].clear()
    without = D._solve_blocks(None, t(u0), t(x0), 0.1, 6, 0)
    for name in readers:
        assert got[name] and all(p is MISSING for p in got[name]), name
    for a, b in zip(with_p, without):
        assert torch.equal(a, b)


# -------------------------------------------------------------------------- public refusals
def test_params_on_unbatched_inputs_is_a_noc_error():
    import noc
    from noc import _lib, problems
    from noc import differential_dynamic_programming as D
    N = 10
    ocp = problems.pendulum(1.0 / N)
    with pytest.raises(_lib.NocError, match="batched"):
        D.interior_point_ddp(ocp, np.zeros((N, 1)), np.array([0.1, -0.1]),
                             params=noc.TrajectoryParams(u_bound=3.0))
    with pytest.raises(_lib.NocError, match="batched"):
        D.ddp(ocp, np.zeros((N, 1)), np.array([0.1, -0.1]), 0.1,
              params=noc.TrajectoryParams(u_bound=3.0))


def test_params_of_another_type_is_a_value_error():
    from noc import problems
    from noc import differential_dynamic_programming as D
    N = 10
    ocp = problems.pendulum(1.0 / N)
    with pytest.raises(ValueError, match="TrajectoryParams"):
        D.interior_point_ddp(ocp, np.zeros((2, N, 1)), np.zeros((2, 2)), params=dict(u_bound=3.0))
    lin8 = problems.double_integrators(4, 0.1, constrained=True)  # the building-block path
    with pytest.raises(ValueError, match="TrajectoryParams"):
        D.interior_point_ddp(lin8, np.zeros((2, N, 4)), np.zeros((2, 8)), params=[1.0])
