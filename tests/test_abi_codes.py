"""The exact return code and message word of every argument error of the C ABI, as one table.

Every row is a call that libnoc_hip.so answers before any HIP call: a rejected argument (-1 bad
value, -2 NULL, -3 misaligned -- the codes include/noc_hip.h lists, the `_params` and `_compact`
forms' own -1 included) or an empty batch (0).  The device addresses (16, 24, ...) are never
dereferenced, so the table reads the same with and without a device.  Two-fault rows pin the
order of the checks.  noc_relayout has no empty-batch return (it launches), so it has no such
row."""
import ctypes
import math

from noc import _lib, problems

P = 16  # a 16-byte aligned fake device address
NAN, INF = float("nan"), float("inf")


def _bad_family():
    f = problems.pendulum(0.02).family
    f.nx = 3
    return f.to_c()


PEND = problems.pendulum(0.02).family.to_c()
CART = problems.cartpole(0.005).family.to_c()
LIN2 = problems.double_integrators(1, 0.1).family.to_c()
LIN8 = problems.double_integrators(4, 0.001).family.to_c()
BAD3 = _bad_family()

WS_REQUIRED = ["x", "u", "x0", "A", "B", "Q", "R", "M", "r", "P", "cx", "cu", "lc", "lam", "dx",
               "du", "pred", "K", "d", "feasible", "phase", "kkt_active", "it", "inner", "total_it",
               "kkt_solves", "bp", "rp", "rinc", "cost", "hu", "gnorm", "reg"]

# illegal lanes next to each set of legal ones
DIMS_BAD = (-1, 2, 7, 9, 15, 17, 31, 33, 63, 65, 127, 129)      # legal 0 1 8 16 32 64 128
RELAYOUT_BAD = (0, 2, 7, 9, 15, 17, 31, 33, 63, 65, 127, 129)   # legal 1 8 16 32 64 128
WS_BAD = (0, 2, 7, 9, 15, 17, 31, 33, 63, 65, 128)              # legal 1 8 16 32 64
COMPACT_BAD = (0, 1, 7, 9, 15, 17, 31, 33, 63, 65, 128)         # legal 8 16 32 64


def W(**over):
    """a valid workspace (Bt 1, N 10, lanes 32, every pointer set) with `over` applied"""
    w = _lib.NocIpmWs()
    w.Bt, w.N, w.lanes, w.flags = 1, 10, 32, 0
    for f in _lib.WS_DOUBLE_FIELDS + _lib.WS_INT_FIELDS + _lib.WS_STATE_FIELDS:
        setattr(w, f, P)
    for k, v in over.items():
        setattr(w, k, v)
    return w


TABLE = []


def rows(fn, base, cases):
    """cases: (overrides of the valid call `base`, exact return code, word of noc_last_error)"""
    for over, code, word in cases:
        assert set(over) <= set(base), (fn, over)
        TABLE.append((fn, dict(base, **over), code, word))


def ptrs(names, **kw):
    return {n: P for n in names.split()} | kw


# ---- the KKT solves ------------------------------------------------------------------------------
KKT_PTRS = "A Bm Q R M r q c P p x0 reg active dx du pred feasible K d S v"
KKT = dict(nx=4, nu=1, N=10, B=1, lanes=32) | ptrs(KKT_PTRS, stream=None)
BWD = dict(nx=4, nu=1, N=10, B=1, lanes=32) | ptrs(
    "A Bm Q R M r q c P p reg active K d S v pred feasible", stream=None)
FWD = dict(nx=4, nu=1, N=10, B=1, lanes=32) | ptrs("A Bm c x0 K d active du dx", stream=None)


def kkt_dims(req):
    return ([(dict(nx=3), -1, "unsupported"), (dict(N=0), -1, "horizon"), (dict(B=-1), -1, "batch"),
             (dict(B=0), 0, ""),
             (dict(nx=3, **{req: None}), -1, "unsupported"), (dict(N=0, **{req: None}), -1, "horizon"),
             (dict(lanes=48, **{req: None}), -1, "lanes")]
            + [(dict(lanes=l), -1, "lanes") for l in DIMS_BAD])


for fn in ("noc_kkt_solve", "noc_kkt_solve_tiled"):
    rows(fn, KKT, kkt_dims("A")
         + [({n: None}, -2, "NULL: " + ("B" if n == "Bm" else n)) for n in "A Bm Q R M r P".split()]
         + [(dict(A=24), -3, "16-byte"), (dict(v=24), -3, "16-byte"), (dict(reg=20), -3, "8-byte"),
            (dict(pred=20), -3, "8-byte"), (dict(feasible=18), -3, "4-byte"),
            (dict(active=18), -3, "4-byte"), (dict(reg=24, pred=40, feasible=20, active=36, B=0), 0, ""),
            (dict(A=None, Q=24), -2, "NULL: A"),   # the ladder's order: A before Q
            (dict(A=24, Bm=None), -3, "16-byte"),
            # gains that do not fit on chip need K and d
            (dict(nx=8, nu=4, N=512, lanes=16, K=None), -2, "noc_kkt_gains_on_chip"),
            (dict(nx=8, nu=4, N=512, lanes=16, d=None), -2, "noc_kkt_gains_on_chip"),
            (dict(nx=8, nu=4, N=512, lanes=16, d=None, B=0), 0, "")])
rows("noc_kkt_solve", KKT, [(dict(lanes=0, B=0), 0, "")])
rows("noc_kkt_solve_tiled", KKT, [
    (dict(lanes=0), -1, "explicit lanes"), (dict(lanes=0, B=0), 0, ""),   # checked after B == 0
    (dict(lanes=1), -1, "grouped"), (dict(lanes=0, K=None), -1, "explicit lanes")])
rows("noc_par_bwd_pass", BWD, kkt_dims("A")
     + [({n: None}, -2, "NULL: " + ("B" if n == "Bm" else n)) for n in "A Bm Q R M r P".split()]
     + [(dict(A=24), -3, "16-byte"), (dict(reg=20), -3, "8-byte"), (dict(feasible=18), -3, "4-byte"),
        (dict(K=None), -2, "noc_kkt_gains_on_chip"), (dict(d=None), -2, "noc_kkt_gains_on_chip")])
rows("noc_par_fwd_pass", FWD, kkt_dims("A")
     + [(dict(A=None), -2, "NULL: A"), (dict(Bm=None), -2, "NULL: B"),
        (dict(A=24), -3, "16-byte"), (dict(active=18), -3, "4-byte"),
        (dict(K=None), -2, "noc_kkt_gains_on_chip"), (dict(d=None), -2, "noc_kkt_gains_on_chip")])
rows("noc_kkt_pick_lanes", dict(nx=4, nu=1, N=10, B=1),
     [(dict(nx=3), -1, "unsupported"), (dict(N=0), -1, "horizon"), (dict(B=-1), -1, "batch"),
      (dict(nx=3, N=0), -1, "unsupported")])

RELAYOUT = dict(direction=0, E=4, sym_n=0, N=10, B=1, lanes=32, src=P, dst=P, stream=None)
rows("noc_relayout", RELAYOUT,
     [(dict(direction=2), -1, "direction"), (dict(direction=-1), -1, "direction"),
      (dict(N=0), -1, "bad dims"), (dict(B=-1), -1, "bad dims"), (dict(E=0), -1, "bad dims"),
      (dict(sym_n=3, E=5), -1, "sym_n"), (dict(src=None), -2, "NULL"), (dict(dst=None), -2, "NULL"),
      (dict(direction=2, N=0), -1, "direction"), (dict(N=0, src=None), -1, "bad dims"),
      (dict(lanes=2, src=None), -1, "lanes")]
     + [(dict(lanes=l), -1, "lanes") for l in RELAYOUT_BAD])

# ---- compact blocks ------------------------------------------------------------------------------
COMPACT = dict(fam=CART, N=10, B=1, lanes=32) | ptrs(
    "A Bm Q R M r P x0 reg active dx du pred feasible K d S v", stream=None)
rows("noc_kkt_solve_compact", COMPACT,
     [(dict(fam=None), -1, "family is NULL"), (dict(fam=LIN8), -1, "compact"),
      (dict(fam=BAD3), -1, "compact"), (dict(N=0), -1, "horizon"), (dict(B=-1), -1, "batch"),
      (dict(B=0), 0, ""), (dict(fam=None, N=0), -1, "family is NULL"),
      (dict(N=0, A=None), -1, "horizon"), (dict(lanes=128, A=None), -1, "lanes")]
     + [(dict(lanes=l), -1, "lanes") for l in COMPACT_BAD]
     + [({n: None}, -1, "NULL: " + ("B" if n == "Bm" else n)) for n in "A Bm Q R M r P".split()]
     + [(dict(A=24), -1, "16-byte"), (dict(x0=24), -1, "16-byte"), (dict(reg=20), -1, "8-byte"),
        (dict(feasible=18), -1, "4-byte"), (dict(reg=24, pred=40, feasible=20, active=36, B=0), 0, ""),
        (dict(N=200, lanes=8, K=None), -1, "noc_kkt_gains_on_chip"),
        (dict(N=200, lanes=8, d=None), -1, "noc_kkt_gains_on_chip"),
        (dict(N=200, lanes=8, d=None, B=0), 0, "")])
EXPAND = dict(fam=CART, N=10, B=1, lanes=32) | ptrs("cA cB cQ cR cM A Bm Q R M", stream=None)
rows("noc_blocks_expand", EXPAND,
     [(dict(fam=None), -1, "family is NULL"), (dict(fam=LIN2), -1, "compact"), (dict(N=0), -1, "horizon"),
      (dict(B=-1), -1, "batch"), (dict(B=0), 0, ""), (dict(fam=None, N=0), -1, "family is NULL"),
      (dict(N=0, cA=None), -1, "horizon"), (dict(cA=24), -1, "16-byte"), (dict(M=24), -1, "16-byte")]
     + [(dict(lanes=l), -1, "lanes") for l in COMPACT_BAD]
     + [({n: None}, -1, "NULL") for n in "cA cB cQ cR cM A Bm Q R M".split()])
rows("noc_compact_width", dict(fam=CART, field=0),
     [(dict(fam=None), -1, "family is NULL"), (dict(field=5), -1, "unsupported"),
      (dict(field=-1), -1, "unsupported"), (dict(fam=LIN8), -1, "unsupported")])
rows("noc_kkt_compact_keep", dict(fam=CART, lanes=32), [(dict(fam=None), -1, "family is NULL")])

# ---- the launch-per-phase interior-point entry points --------------------------------------------


def ws_rows(fam, bad=WS_BAD, lanes=32, null=-2, ptr=-2, val=-1, grouped=True):
    """the workspace checks shared by every noc_ipm_* entry point (check order: dims, lanes, the
    grouped layout, the family, the pointers, the flags)"""
    out = [(dict(ws=None), null, "NULL"), (dict(ws=W(lanes=lanes, Bt=-1)), val, "dims"),
           (dict(ws=W(lanes=lanes, N=0)), val, "dims"), (dict(ws=W(lanes=lanes, flags=8)), val, "flags"),
           (dict(ws=W(lanes=lanes, flags=7, Bt=0)), 0, ""), (dict(ws=W(lanes=lanes, Bt=0)), 0, ""),
           (dict(ws=W(lanes=lanes, N=0, x=None)), val, "dims"),
           (dict(ws=W(lanes=lanes, x=None, flags=8)), ptr, "pointer is NULL"),
           (dict(ws=W(lanes=lanes, repeats=None, Bt=0)), 0, "")]
    out += [(dict(ws=W(lanes=l)), val, "lanes") for l in bad]
    out += [(dict(ws=W(lanes=lanes, **{n: None})), ptr, "pointer is NULL") for n in WS_REQUIRED]
    if fam:
        out += [(dict(fam=None), null, "NULL"), (dict(fam=BAD3), val, "unsupported"),
                (dict(fam=None, ws=W(lanes=lanes, N=0)), null, "NULL"),
                (dict(ws=W(lanes=1)), val, "grouped"),
                (dict(fam=BAD3, ws=W(lanes=lanes, x=None)), val, "unsupported")]
        if grouped:  # the grouped layout of nx = 8
            out += [(dict(fam=LIN8, ws=W(lanes=1, Bt=0)), 0, "")]
    return out


MODE = [(dict(mode=2), -1, "bad mode"), (dict(mode=-1), -1, "bad mode")]
TERMINAL = [(dict(terminal=2), -1, "terminal"), (dict(terminal=-1), -1, "terminal"),
            (dict(mode=2, terminal=2), -1, "bad mode")]
LANES_ARG = [(dict(lanes=64), -1, "differs"), (dict(lanes=31), -1, "differs"),
             (dict(lanes=33), -1, "differs"), (dict(lanes=0, ws=W(Bt=0)), 0, ""),
             (dict(lanes=32, ws=W(Bt=0)), 0, "")]

rows("noc_ipm_init", dict(ws=W(), bp0=0.1, stream=None),
     ws_rows(False)
     + [(dict(ws=W(lanes=1, Bt=0)), 0, ""),
        (dict(ws=W(Bt=0), bp0=-1.0), 0, ""), (dict(ws=W(Bt=0), bp0=NAN), 0, "")])
rows("noc_ipm_promote", dict(ws=W(), stream=None), ws_rows(False))
rows("noc_ipm_rollout", dict(fam=PEND, ws=W(), stream=None), ws_rows(True))
rows("noc_ipm_trial", dict(fam=PEND, ws=W(), mode=0, stream=None),
     ws_rows(True) + MODE + [(dict(fam=None, mode=2), -2, "family"), (dict(ws=W(x=None), mode=2), -2, "NULL")])
for fn in ("noc_ipm_prepare", "noc_ipm_step_main"):
    rows(fn, dict(fam=PEND, ws=W(), mode=0, terminal=0, stream=None),
         ws_rows(True) + MODE + TERMINAL
         + [(dict(fam=None, mode=2), -2, "family"), (dict(ws=W(flags=8), terminal=2), -1, "flags")])
# the step forms' KKT solve checks the workspace's fields as its own arguments (also at Bt = 0)
WS_ALIGN = [(dict(ws=W(Bt=0, A=24)), "16-byte"), (dict(ws=W(Bt=0, dx=24)), "16-byte"),
            (dict(ws=W(Bt=0, reg=20)), "8-byte"), (dict(ws=W(Bt=0, feasible=18)), "4-byte"),
            (dict(ws=W(Bt=0, kkt_active=18)), "4-byte")]
rows("noc_ipm_step", dict(fam=PEND, ws=W(), mode=0, terminal=0, lanes=0, stream=None),
     ws_rows(True) + MODE + TERMINAL + LANES_ARG + [(o, -3, w) for o, w in WS_ALIGN]
     + [(dict(fam=None, lanes=64), -1, "differs"), (dict(ws=None, lanes=64), -2, "workspace"),
        (dict(ws=W(x=None), lanes=64), -1, "differs")])

# the _compact forms: -1 for a NULL family or workspace, then their dense twins' codes
for fn in ("noc_ipm_prepare_compact", "noc_ipm_step_main_compact"):
    rows(fn, dict(fam=CART, ws=W(), mode=0, terminal=0, stream=None),
         ws_rows(True, null=-1, grouped=False) + MODE + TERMINAL
         + [(dict(fam=LIN2), -1, "compact"), (dict(fam=LIN2, mode=2), -1, "compact"),
            (dict(fam=LIN2, ws=W(flags=8)), -1, "flags")])
rows("noc_ipm_step_compact", dict(fam=CART, ws=W(), mode=0, terminal=0, lanes=0, stream=None),
     ws_rows(True, null=-1, grouped=False) + MODE + TERMINAL + LANES_ARG + [(o, -1, w) for o, w in WS_ALIGN]
     + [(dict(fam=LIN2), -1, "compact"), (dict(fam=None, lanes=64), -1, "NULL"),
        (dict(ws=None, lanes=64), -1, "NULL")])

# ---- the persistent solve ------------------------------------------------------------------------
SOLVE = dict(fam=CART, ws=W(lanes=64), mode=0, terminal=0, bp0=0.1, max_solves=100, stream=None)
SOLVE_VALUES = [(dict(bp0=0.0), -1, "bp0"), (dict(bp0=-1.0), -1, "bp0"), (dict(bp0=NAN), -1, "bp0"),
                (dict(bp0=INF, ws=W(lanes=64, Bt=0)), 0, ""),    # inf > 0: accepted
                (dict(max_solves=0), -1, "max_solves"), (dict(max_solves=-1), -1, "max_solves"),
                (dict(bp0=0.0, max_solves=0), -1, "bp0"), (dict(terminal=2, bp0=0.0), -1, "terminal")]
rows("noc_ipm_solve", SOLVE,
     ws_rows(True, bad=(63, 65), lanes=64, grouped=False) + MODE + TERMINAL + SOLVE_VALUES
     + [(dict(ws=W(lanes=32)), -1, "lanes = 64"), (dict(ws=W(lanes=8)), -1, "lanes = 64"),
        (dict(ws=W(lanes=64, N=2000)), -1, "noc_ipm_solve_supported"),
        (dict(fam=LIN8, ws=W(lanes=64)), -1, "noc_ipm_solve_supported"),
        (dict(ws=W(lanes=32), max_solves=0), -1, "max_solves")])
PLAN_OUT = (ctypes.c_int * _lib.PLAN_INTS)()
rows("noc_debug_ipm_plan", dict(fam=CART, N=10, Bt=1, flags=0, ordered=0, with_params=0, simds=1024,
                                out=PLAN_OUT, n=_lib.PLAN_INTS),
     [(dict(fam=None), -2, "NULL"), (dict(out=None), -2, "NULL"), (dict(n=17), -1, "NOC_PLAN_INTS"),
      (dict(N=0), -1, "N >= 1"), (dict(Bt=-1), -1, "Bt >= 0"), (dict(simds=-1), -1, "simds"),
      (dict(flags=8), -1, "flags"), (dict(flags=7), 0, ""), (dict(Bt=0), 0, ""), (dict(fam=BAD3), 0, ""),
      (dict(fam=None, N=0), -2, "NULL"), (dict(N=0, out=None), -2, "NULL"), (dict(n=17, N=0), -1, "NOC_PLAN_INTS"),
      (dict(N=0, flags=8), -1, "N >= 1")])
HOST_OUT = (ctypes.c_longlong * 32)()
rows("noc_debug_phase_cycles", dict(out=HOST_OUT, n=16, reset=0),
     [(dict(out=None), -2, "NULL"), (dict(n=-1), -2, "NULL")])
rows("noc_debug_traj_times", dict(out=HOST_OUT, n=16), [(dict(out=None), -2, "NULL"), (dict(n=-1), -2, "NULL")])

# ---- per-trajectory parameters: every argument error is -1 ---------------------------------------
PARAMS = [(dict(params=None), -1, "params is NULL"), (dict(params=P + 8), -1, "aligned"),
          (dict(fam=None, params=None), -1, "NULL"), (dict(params=None, fam=BAD3), -1, "params is NULL"),
          (dict(params=P + 8, fam=BAD3), -1, "aligned")]


def ws_params_rows(lanes=32, bad=COMPACT_BAD):
    """check_params: family / workspace NULL, params, the family, the flags, the lanes or horizon
    (noc_traj_params_supported), then the workspace checks of the twin -- all -1"""
    out = [c for c in ws_rows(True, bad=(), lanes=lanes, null=-1, ptr=-1)
           if c[0].get("ws") is None or (c[0]["ws"].lanes != 1 and c[0]["ws"].N != 0
                                         and not (c[0]["ws"].flags == 8 and not c[0]["ws"].x))]
    out += [(dict(ws=W(lanes=l)), -1, "wrong lanes") for l in bad]
    out += [(dict(ws=W(lanes=lanes, N=0)), -1, "horizon"), (dict(ws=W(lanes=lanes, N=0, x=None)), -1, "horizon"),
            (dict(fam=None, ws=W(lanes=lanes, N=0)), -1, "NULL"),
            (dict(ws=W(lanes=lanes, N=0, flags=8)), -1, "flags"),
            (dict(ws=W(lanes=lanes, x=None, flags=8)), -1, "flags"),   # the flags before the pointers
            (dict(fam=BAD3, ws=W(lanes=7)), -1, "unsupported")]
    return out + PARAMS


rows("noc_ipm_trial_params", dict(fam=PEND, ws=W(), params=P, mode=0, stream=None),
     ws_params_rows()
     + MODE + [(dict(ws=W(lanes=7, flags=8)), -1, "flags"), (dict(params=None, mode=2), -1, "params is NULL"),
               (dict(fam=LIN8, ws=W(lanes=1, Bt=0)), 0, "")])
rows("noc_ipm_prepare_params", dict(fam=PEND, ws=W(), params=P, mode=0, terminal=0, stream=None),
     ws_params_rows()
     + MODE + TERMINAL + [(dict(ws=W(lanes=7, flags=8)), -1, "flags"),
                          (dict(params=None, mode=2), -1, "params is NULL")])
rows("noc_ipm_step_params", dict(fam=PEND, ws=W(), params=P, mode=0, terminal=0, lanes=0, stream=None),
     ws_params_rows()
     + MODE + TERMINAL + LANES_ARG + [(o, -3, w) for o, w in WS_ALIGN]   # the KKT solve's own code
     + [(dict(ws=W(lanes=7, flags=8)), -1, "flags"), (dict(params=None, lanes=64), -1, "differs"),
        (dict(fam=None, lanes=64), -1, "differs"), (dict(ws=None, lanes=64), -1, "NULL")])
rows("noc_ipm_solve_params", dict(fam=CART, ws=W(lanes=64), params=P, mode=0, terminal=0, bp0=0.1,
                                  max_solves=100, stream=None),
     ws_params_rows(lanes=64, bad=(0, 1, 8, 16, 32, 63, 65, 128))
     + MODE + TERMINAL + SOLVE_VALUES
     + [(dict(ws=W(lanes=7, flags=8)), -1, "lanes = 64"), (dict(ws=W(lanes=32)), -1, "lanes = 64"),
        (dict(ws=W(lanes=32), params=None), -1, "params is NULL"),
        (dict(ws=W(lanes=32, flags=8)), -1, "lanes = 64"),
        (dict(ws=W(lanes=64, N=2000)), -1, "noc_ipm_solve_supported")])

# ---- the building blocks and interior-point DDP --------------------------------------------------


def block_rows(ptr_names, opt=(), fam=True, N=True, c=(-2, -3), dims="need"):
    """family, N, B, then each pointer NULL / misaligned in turn.  c: the codes of a NULL and of
    a misaligned pointer (the _params forms: -1 for both)"""
    names = ptr_names.split()
    out = [(dict(B=-1), -1, dims), (dict(B=0), 0, ""), (dict(B=-1, **{names[0]: None}), -1, dims),
           ({names[0]: None, names[1]: P + 2}, c[0], "NULL"), ({names[0]: P + 2, names[1]: None}, c[1], "aligned")]
    out += [({n: None}, 0 if n in opt else c[0], "" if n in opt else "NULL") for n in names]
    if N:
        out += [(dict(N=0), -1, dims), (dict(N=0, **{names[0]: None}), -1, dims)]
    if fam:
        out += [(dict(fam=None), -2 if c[0] == -2 else -1, "family is NULL"), (dict(fam=BAD3), -1, "unsupported"),
                (dict(fam=BAD3, **{names[0]: None}), -1, "unsupported")]
        if N:
            out += [(dict(fam=None, N=0), -2 if c[0] == -2 else -1, "family is NULL")]
    return [(o if "B" in o or code != 0 else dict(o, B=0), code, w) for o, code, w in out]


def misaligned(cases, c=-3):
    return [({n: P + off}, c, word) for n, off, word in cases]


DERIV_PTRS = "x u bp cx cu cxx cuu cxu fx fu fxx fuu fxu"
rows("noc_derivatives", dict(fam=PEND, N=10, B=1) | ptrs(DERIV_PTRS, stream=None),
     block_rows(DERIV_PTRS) + misaligned([("x", 4, "8-byte"), ("fxu", 4, "8-byte")])
     + [(dict(x=P + 8, B=0), 0, "")])
rows("noc_final_cost_derivs", dict(fam=PEND, B=1) | ptrs("xN grad hess", stream=None),
     block_rows("xN grad hess", opt=("hess",), N=False)
     + misaligned([("xN", 4, "8-byte"), ("hess", 4, "8-byte")]))
rows("noc_check_feasibility", dict(fam=PEND, N=10, B=1) | ptrs("x u feasible", stream=None),
     block_rows("x u feasible") + misaligned([("x", 4, "8-byte"), ("feasible", 2, "4-byte")])
     + [(dict(feasible=P + 4, B=0), 0, "")])
rows("noc_total_cost", dict(fam=PEND, N=10, B=1) | ptrs("x u bp cost", stream=None),
     block_rows("x u bp cost") + misaligned([("x", 4, "8-byte"), ("cost", 4, "8-byte")]))
rows("noc_nonlin_rollout", dict(fam=PEND, N=10, B=1) | ptrs("K k x u x_new u_new", stream=None),
     block_rows("K k x u x_new u_new") + misaligned([("K", 4, "8-byte"), ("u_new", 4, "8-byte")]))
rows("noc_costates", dict(nx=4, N=10, B=1) | ptrs("lamT cx fx lam", sequential=0, stream=None),
     block_rows("lamT cx fx lam", fam=False) + misaligned([("lamT", 4, "8-byte"), ("lam", 4, "8-byte")])
     + [(dict(nx=0), -1, "nx"), (dict(nx=9), -1, "nx"), (dict(nx=9, N=0), -1, "nx"),
        (dict(nx=0, lamT=None), -1, "nx"), (dict(nx=3, B=0), 0, "")])
LQR_PTRS = "lam cu cxx cuu cxu fu fxx fuu fxu ru Q R M"
rows("noc_lqr_params", dict(nx=4, nu=1, N=10, B=1) | ptrs(LQR_PTRS, stream=None),
     block_rows(LQR_PTRS, fam=False) + misaligned([("lam", 4, "8-byte"), ("M", 4, "8-byte")])
     + [(dict(nx=0), -1, "nx"), (dict(nx=9), -1, "nx"), (dict(nu=0), -1, "nx"), (dict(nu=9), -1, "nx"),
        (dict(nx=9, N=0), -1, "nx"), (dict(nx=0, lam=None), -1, "nx"), (dict(nx=3, B=0), 0, "")])
BWD_PTRS = "Vx Vxx reg_param cx cu cxx cuu cxu fx fu fxx fuu fxu k K pred feasible Hu"
rows("noc_ddp_bwd_pass", dict(nx=4, nu=1, N=10, B=1) | ptrs(BWD_PTRS, stream=None),
     block_rows(BWD_PTRS, fam=False)
     + misaligned([("Vx", 4, "8-byte"), ("Hu", 4, "8-byte"), ("feasible", 2, "4-byte")])
     + [(dict(nx=3), -1, "unsupported"), (dict(nx=3, N=0), -1, "unsupported"),
        (dict(nx=3, Vx=None), -1, "unsupported"), (dict(feasible=P + 4, B=0), 0, ""),
        (dict(feasible=None, Hu=None), -2, "ddp_bwd_pass argument")])  # feasible is checked last

DDP_PTRS = "x0 u work iterations passes done"
DDP = dict(fam=PEND, N=10, Bt=1) | ptrs(DDP_PTRS, bp0=0.1, max_passes=10, stream=None)


def ddp_rows(c=(-2, -3)):
    fam_null = -2 if c[0] == -2 else -1
    return ([(dict(N=0), -1, "horizon"), (dict(Bt=-1), -1, "batch"), (dict(Bt=0), 0, ""),
             (dict(fam=None), fam_null, "family is NULL"), (dict(fam=None, N=0), fam_null, "family is NULL"),
             (dict(fam=LIN8), -1, "nx <= 4"), (dict(N=0, x0=None), -1, "horizon"),
             (dict(bp0=0.0, Bt=0), 0, ""), (dict(bp0=-0.5), -1, "bp0"), (dict(bp0=NAN), -1, "bp0"),
             (dict(bp0=INF), -1, "bp0"), (dict(bp0=-INF), -1, "bp0"), (dict(max_passes=0), -1, "max_passes"),
             (dict(bp0=NAN, max_passes=0), -1, "bp0"), (dict(max_passes=0, x0=None), -1, "max_passes"),
             (dict(x0=None, u=P + 4), c[0], "x0"), (dict(x0=P + 4, u=None), c[1], "x0"),
             (dict(x0=P + 8, u=P + 24, work=P + 40, iterations=P + 4, passes=P + 20, done=P + 36, Bt=0), 0, "")]
            + [({n: None}, c[0], "NULL: " + n) for n in DDP_PTRS.split()]
            + misaligned([("x0", 4, "8-byte"), ("work", 4, "8-byte"), ("iterations", 2, "4-byte"),
                          ("done", 2, "4-byte")], c[1]))


rows("noc_ddp_solve", DDP, ddp_rows() + [(dict(fam=BAD3), -1, "noc_ddp_supported")])
rows("noc_ddp_solve_ex", dict(fam=PEND, N=10, Bt=1) | ptrs(DDP_PTRS, bp0=0.1, max_passes=10, flags=0,
                                                            stream=None),
     ddp_rows() + [(dict(fam=BAD3), -1, "noc_ddp_supported"), (dict(flags=2), -1, "flags"),
                   (dict(flags=3), -1, "flags"), (dict(flags=1, Bt=0), 0, ""),
                   (dict(flags=2, fam=None), -1, "flags"), (dict(flags=2, N=0), -1, "flags")])

# the _params building blocks: the params prefix, then the twin's checks, every code -1
BLOCK_PARAMS = PARAMS + [(dict(fam=None), -1, "family is NULL"), (dict(fam=BAD3), -1, "unsupported family")]
M1 = (-1, -1)
rows("noc_derivatives_params", dict(fam=PEND, N=10, B=1) | ptrs(DERIV_PTRS, params=P, stream=None),
     block_rows(DERIV_PTRS, c=M1) + misaligned([("x", 4, "8-byte"), ("fxu", 4, "8-byte")], -1)
     + BLOCK_PARAMS + [(dict(params=None, N=0), -1, "params is NULL"), (dict(fam=LIN8, B=0), 0, "")])
rows("noc_final_cost_derivs_params", dict(fam=PEND, B=1) | ptrs("xN grad hess", params=P, stream=None),
     block_rows("xN grad hess", opt=("hess",), N=False, c=M1)
     + misaligned([("xN", 4, "8-byte"), ("hess", 4, "8-byte")], -1)
     + BLOCK_PARAMS + [(dict(params=None, B=-1), -1, "params is NULL")])
rows("noc_check_feasibility_params", dict(fam=PEND, N=10, B=1) | ptrs("x u feasible", params=P, stream=None),
     block_rows("x u feasible", c=M1) + misaligned([("x", 4, "8-byte"), ("feasible", 2, "4-byte")], -1)
     + BLOCK_PARAMS + [(dict(params=None, N=0), -1, "params is NULL")])
rows("noc_total_cost_params", dict(fam=PEND, N=10, B=1) | ptrs("x u bp cost", params=P, stream=None),
     block_rows("x u bp cost", c=M1) + misaligned([("x", 4, "8-byte"), ("cost", 4, "8-byte")], -1)
     + BLOCK_PARAMS + [(dict(params=None, N=0), -1, "params is NULL")])
DDP_PARAMS = dict(fam=PEND, N=10, Bt=1) | ptrs(DDP_PTRS, params=P, bp0=0.1, max_passes=10, flags=0,
                                               stream=None)
rows("noc_ddp_solve_params", DDP_PARAMS,
     [c for c in ddp_rows(M1) if c[0].get("fam") is not LIN8]
     + BLOCK_PARAMS + [(dict(fam=LIN8), -1, "noc_ddp_params_supported"), (dict(flags=2), -1, "flags"),
                       (dict(flags=1, Bt=0), 0, ""), (dict(flags=2, params=None), -1, "params is NULL"),
                       (dict(flags=2, N=0), -1, "flags"), (dict(params=None, N=0), -1, "params is NULL")])


def _arg(v):
    return ctypes.byref(v) if isinstance(v, (_lib.NocFamily, _lib.NocIpmWs)) else v


def _batch(args):
    if "ws" in args:
        return args["ws"].Bt
    return args.get("B", args.get("Bt"))


def _show(v):
    if isinstance(v, _lib.NocIpmWs):
        return "ws(Bt=%d,N=%d,lanes=%d,flags=%d%s)" % (
            v.Bt, v.N, v.lanes, v.flags, "".join("," + n + "=NULL" for n in WS_REQUIRED if not getattr(v, n)))
    if isinstance(v, _lib.NocFamily):
        return "fam(kind=%d,nx=%d)" % (v.kind, v.nx)
    return repr(v)


def test_every_entry_point_has_rows():
    """every function of the header that returns a status is in the table"""
    status = {n for n, (res, args) in _lib.SIGNATURES.items() if res is ctypes.c_int and args} - {
        # queries: they answer 0 / 1 (or a count) and set no error
        "noc_kkt_supported", "noc_kkt_default_lanes", "noc_kkt_gains_on_chip", "noc_family_supported",
        "noc_kkt_compact_supported", "noc_ipm_solve_supported", "noc_traj_params_supported",
        "noc_ddp_supported", "noc_ddp_params_supported"}
    assert status == {fn for fn, _, _, _ in TABLE}


def test_rows_stop_before_any_device_call():
    """a row is a rejection (-1 / -2 / -3) or a call on an empty batch: never a launch"""
    for fn, args, code, word in TABLE:
        assert code in (-1, -2, -3) or (code == 0 and (_batch(args) == 0 or fn == "noc_debug_ipm_plan")), (fn, args)
        assert code == 0 or word, (fn, args)
        assert not any(isinstance(v, float) and math.isinf(v) for v in args.values()) or code != 0 \
            or _batch(args) == 0


def test_return_codes_and_messages():
    lib = _lib.load()
    wrong = []
    for fn, args, code, word in TABLE:
        rc = getattr(lib, fn)(*(_arg(v) for v in args.values()))
        msg = lib.noc_last_error().decode()
        if rc != code or (code != 0 and word not in msg):
            wrong.append("%s(%s): want %d '%s', got %d '%s'" % (
                fn, ", ".join("%s=%s" % (k, _show(v)) for k, v in args.items()), code, word, rc, msg))
    assert not wrong, "%d of %d rows:\n%s" % (len(wrong), len(TABLE), "\n".join(wrong))
