"""Per-trajectory cost parameters, host side (no GPU): the additive C-ABI entry points exist and
refuse bad arguments before any device call, and noc.TrajectoryParams packs against a Family into
the (Bt, 32) record of include/noc_hip.h."""
import ctypes

import numpy as np
import pytest

NEW_SYMBOLS = ["noc_traj_params_supported", "noc_ipm_solve_params", "noc_ipm_prepare_params",
               "noc_ipm_trial_params", "noc_ipm_step_params"]


def _lib_and_problems():
    from noc import _lib, problems
    return _lib, _lib.load(), problems


def _fake_ws(_lib, Bt=4, N=40, lanes=64):
    """a workspace of non-NULL fake pointers: argument checks run before any device call"""
    ws = _lib.NocIpmWs()
    ws.Bt, ws.N, ws.lanes = Bt, N, lanes
    for f in _lib.WS_DOUBLE_FIELDS + _lib.WS_INT_FIELDS + _lib.WS_STATE_FIELDS:
        setattr(ws, f, 256)
    return ws


def test_symbols_exist_and_the_abi_version_is_unchanged():
    _lib, lib, _ = _lib_and_problems()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert lib.noc_abi_version() == 5


def test_supported_query():
    _lib, lib, problems = _lib_and_problems()
    sup = lambda fam, N, lanes: lib.noc_traj_params_supported(ctypes.byref(fam), N, lanes)
    for ocp in (problems.pendulum(0.02), problems.cartpole(0.005), problems.double_integrators(1, 0.1)):
        assert sup(ocp.family.to_c(), 40, 64) == 1
    lin8 = problems.double_integrators(4, 0.001).family.to_c()
    assert (lin8.nx, lin8.nu) == (8, 4)
    assert sup(lin8, 24, 1) == 1 and sup(lin8, 24, 16) == 1   # launch-per-phase lane counts
    cart = problems.cartpole(0.005).family.to_c()
    assert sup(cart, 40, 1) == 0      # the grouped layout is the (8, 4) family's
    assert sup(cart, 40, 128) == 0
    assert sup(cart, 0, 64) == 0
    bad = problems.pendulum(0.02).family.to_c()
    bad.kind = 77
    assert sup(bad, 40, 64) == 0
    assert lib.noc_traj_params_supported(None, 40, 64) == 0


def test_argument_errors_return_minus_one_with_a_message():
    _lib, lib, problems = _lib_and_problems()
    cart = problems.cartpole(0.005).family.to_c()
    fam, P = ctypes.byref(cart), 4096  # P: a fake, aligned, non-NULL record pointer

    def calls(f, ws, p, lanes=0):
        w = ctypes.byref(ws)
        return {"solve": lambda: lib.noc_ipm_solve_params(f, w, p, 0, 1, 0.1, 100, None),
                "prepare": lambda: lib.noc_ipm_prepare_params(f, w, p, 0, 1, None),
                "trial": lambda: lib.noc_ipm_trial_params(f, w, p, 0, None),
                "step": lambda: lib.noc_ipm_step_params(f, w, p, 0, 1, lanes, None)}

    def refused(fn, word):
        assert fn() == -1
        assert word in lib.noc_last_error(), lib.noc_last_error()

    ws = _fake_ws(_lib)
    for fn in calls(fam, ws, None).values():           # NULL params
        refused(fn, b"params is NULL")
    bad = problems.cartpole(0.005).family.to_c()
    bad.kind = 77
    for fn in calls(ctypes.byref(bad), ws, P).values():  # an unsupported family
        refused(fn, b"unsupported family")
    ws32 = _fake_ws(_lib, lanes=32)
    refused(calls(fam, ws32, P)["solve"], b"lanes")      # the persistent solve needs lanes 64
    refused(calls(fam, ws32, P, lanes=64)["step"], b"lanes")  # lanes differ from the workspace's
    ws128 = _fake_ws(_lib, lanes=128)
    for name in ("prepare", "trial", "step"):
        refused(calls(fam, ws128, P)[name], b"lanes")
    wsf = _fake_ws(_lib)
    wsf.flags = 1 << 6
    for fn in calls(fam, wsf, P).values():               # an unknown flag bit
        refused(fn, b"flags")


# ------------------------------------------------------------------------------------ packing
def _pack(params, fam, Bt):
    from noc.traj_params import pack
    return pack(params, fam, Bt)


def test_pack_defaults_come_from_the_family():
    import noc
    from noc import problems
    fam = problems.cartpole(0.005).family
    rec = _pack(noc.TrajectoryParams(), fam, 3)
    assert rec.shape == (3, 32) and rec.dtype == np.float64
    for b in range(3):
        assert np.array_equal(rec[b, 0:4], np.asarray(fam.goal, dtype=np.float64))
        assert np.array_equal(rec[b, 8:12], np.asarray(fam.wx, dtype=np.float64))
        assert np.array_equal(rec[b, 16:17], np.asarray(fam.wu, dtype=np.float64))
        assert np.array_equal(rec[b, 20:24], np.asarray(fam.wf, dtype=np.float64))
        assert rec[b, 28] == fam.u_bound
    # entries past nx / nu and the reserved tail are zero
    assert not rec[:, 4:8].any() and not rec[:, 12:16].any() and not rec[:, 17:20].any()
    assert not rec[:, 24:28].any() and not rec[:, 29:].any()


def test_pack_broadcasts_a_row_and_keeps_per_trajectory_rows():
    import noc
    from noc import problems
    fam = problems.cartpole(0.005).family
    goal = np.arange(12, dtype=np.float64).reshape(3, 4) + 0.5
    wu = np.array([0.25])
    ub = np.array([3.0, 4.0, 5.0])
    rec = _pack(noc.TrajectoryParams(goal=goal, wu=wu, u_bound=ub), fam, 3)
    assert np.array_equal(rec[:, 0:4], goal)             # (Bt, n): row for row
    assert np.array_equal(rec[:, 16], np.full(3, 0.25))  # (n,): every row
    assert np.array_equal(rec[:, 28], ub)
    assert np.array_equal(rec[:, 8:12], np.tile(np.asarray(fam.wx, dtype=np.float64), (3, 1)))
    rec = _pack(noc.TrajectoryParams(u_bound=2.5), fam, 3)  # a scalar bound
    assert np.array_equal(rec[:, 28], np.full(3, 2.5))
    # rows(): what a shard of the batch is solved with
    part = noc.TrajectoryParams(goal=goal, wu=wu, u_bound=ub).rows(1, 3)
    assert np.array_equal(_pack(part, fam, 2), _pack(noc.TrajectoryParams(goal=goal, wu=wu, u_bound=ub),
                                                     fam, 3)[1:3])


def test_pack_refuses_bad_fields():
    import noc
    from noc import problems
    cart = problems.cartpole(0.005).family
    assert cart.u_bound > 0
    T = noc.TrajectoryParams
    for bad in (T(goal=np.zeros(3)), T(goal=np.zeros((2, 4))), T(wu=np.zeros((3, 2))),
                T(wf=np.zeros((3, 4, 1))), T(u_bound=np.ones(2)), T(u_bound=np.ones((3, 1)))):
        with pytest.raises(ValueError, match="shape"):
            _pack(bad, cart, 3)
    for bad in (T(wx=[1.0, np.nan, 1.0, 1.0]), T(goal=np.full((3, 4), np.inf)), T(u_bound=np.nan)):
        with pytest.raises(ValueError, match="non-finite"):
            _pack(bad, cart, 3)
    for bad in (T(u_bound=0.0), T(u_bound=[1.0, -2.0, 1.0])):
        with pytest.raises(ValueError, match="> 0"):
            _pack(bad, cart, 3)
    free = problems.double_integrators(1, 0.1).family   # unconstrained: no barrier to move
    if free.u_bound > 0:
        free = problems.double_integrators(1, 0.1, constrained=False).family
    assert not free.u_bound > 0
    with pytest.raises(ValueError, match="without a control bound"):
        _pack(T(u_bound=1.0), free, 3)
    with pytest.raises(ValueError):
        _pack(dict(goal=None), cart, 3)
