"""Generate the committed golden fixtures (test infrastructure).

The reference cannot run here (pure JAX; jax/jaxlib/paroc absent, no network), so the fixtures
are produced by the oracle restatement (oracle/noc_oracle.py) and cross-checked at generation
time against the dense KKT solve.  They pin the oracle against regressions and give the GPU
tests fixed vectors that do not depend on re-running the oracle.  Run from the repo root:
    python tests/golden/make_golden.py [--v2-only | --v3-only]
golden_v3 (whole solves for the schedule tests) takes minutes of CPU; --v3-only writes only it.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from lq_cases import rand_lq, oracle_batch  # noqa: E402
from oracle import noc_oracle as O, problems as PR  # noqa: E402


def lq_fixtures():
    out = {}
    for nx, nu, N in [(2, 1, 50), (4, 1, 120), (8, 4, 48)]:
        for aff in (False, True):
            tag = f"lq_{nx}x{nu}_N{N}_{'aff' if aff else 'newton'}"
            case = rand_lq(7 + nx * 100 + N + int(aff), 2, N, nx, nu, affine=aff)
            ref = oracle_batch(case)
            for b in range(2):
                g = lambda k: None if k not in case else case[k][b]
                ddx, ddu, _ = O.dense_kkt(g("A"), g("B"), g("Q"), g("R"), g("M"), g("r"), g("P"),
                                          g("reg"), g("x0"), g("q"), g("c"), g("p"))
                assert np.max(np.abs(ddx - ref["dx"][b])) < 1e-10 * max(1, np.abs(ddx).max())
                assert np.max(np.abs(ddu - ref["du"][b])) < 1e-10 * max(1, np.abs(ddu).max())
            for k, v in case.items():
                out[f"{tag}/in/{k}"] = v
            for k, v in ref.items():
                out[f"{tag}/out/{k}"] = np.asarray(v)
    return out


def ipm_fixtures():
    out = {}
    N = 50
    prob = O.NumpyProblem(PR.pendulum_ocp(1.0 / N))
    u0 = 0.1 * np.random.default_rng(1).normal(size=(N, 1))
    x0 = np.array([0.1, -0.1])
    U, it, solves = O.par_interior_point_optimal_control(prob, u0, x0)
    Us, its = O.seq_interior_point_optimal_control(prob, u0, x0)
    out.update({"pend50/u0": u0, "pend50/x0": x0, "pend50/par_u": U,
                "pend50/par_iters": np.array(it), "pend50/par_kkt_solves": np.array(solves),
                "pend50/seq_u": Us, "pend50/seq_iters": np.array(its),
                "pend50/par_cost": np.array(prob.total_cost(O.rollout(prob.dynamics, U, x0), U, 0.0))})
    # one linearisation of cart-pole (N=20) at a random iterate: the LQ blocks of the first step
    N = 20
    prob = O.NumpyProblem(PR.cartpole_ocp(1.0 / N))
    rng = np.random.default_rng(4)
    u = 0.1 * rng.normal(size=(N, 1))
    x0 = np.array([0.01, 2 * np.pi - 0.01, 0.01, -0.01])
    X = O.rollout(prob.dynamics, u, x0)
    L = O.linearize(prob, X, u, 0.1)
    out.update({"cart20/u": u, "cart20/x": X})
    for k in ("A", "B", "Q", "R", "M", "r", "P", "cu", "lam"):
        out[f"cart20/{k}"] = L[k]
    out["cart20/cost"] = np.array(prob.total_cost(X, u, 0.1))
    return out


def newton_block_fixtures():
    """golden_v2: the LQ blocks of a real first Newton step (bp = 0.1, rp = 1, so
    reg = ||cu||_F, P:116-118) of the BASELINE problems -- pendulum N=100 (c2) and cart-pole
    N=200 (c3), two trajectories each from the SURVEY §8d input distributions -- linearised by
    the autodiff oracle (P:13-42), and the KKT step of each computed by the FAITHFUL sequential
    Riccati (S:42-90: Vxx propagated unsymmetrised, inv(Quu), eigh test), checked against the
    dense KKT solve at generation time.  The GPU tests compare the HIP path with these committed
    vectors directly (no live oracle)."""
    out = {}
    cases = [("pend100", PR.pendulum_ocp(1.0 / 100), 100, "pendulum"),
             ("cart200", PR.cartpole_ocp(1.0 / 200), 200, "cartpole")]
    for tag, tocp, N, name in cases:
        prob = O.NumpyProblem(tocp)
        rng = np.random.default_rng(2024 + N)
        if name == "pendulum":
            x0s = np.array([0.1, -0.1]) + 0.01 * rng.normal(size=(2, 2))
        else:
            x0s = np.array([0.01, 2 * np.pi - 0.01, 0.01, -0.01]) + 0.01 * rng.normal(size=(2, 4))
        u0s = 0.1 * rng.normal(size=(2, N, 1))
        blocks = {k: [] for k in ("x", "A", "B", "Q", "R", "M", "r", "P", "reg", "dx", "du", "pred",
                                  "feasible", "K", "d")}
        for b in range(2):
            X = O.rollout(prob.dynamics, u0s[b], x0s[b])
            L = O.linearize(prob, X, u0s[b], 0.1)
            reg = float(np.linalg.norm(L["cu"]))
            dx, du, pred, feas, K, d, S, v = O.kkt_solve(L["A"], L["B"], L["Q"], L["R"], L["M"],
                                                         L["r"], L["P"], reg, symmetrize=False)
            ddx, ddu, _ = O.dense_kkt(L["A"], L["B"], L["Q"], L["R"], L["M"], L["r"], L["P"], reg)
            assert np.max(np.abs(ddx - dx)) < 1e-10 * max(1, np.abs(ddx).max())
            assert np.max(np.abs(ddu - du)) < 1e-10 * max(1, np.abs(ddu).max())
            for k, val in (("x", X), ("reg", reg), ("dx", dx), ("du", du), ("pred", pred),
                           ("feasible", feas), ("K", K), ("d", d)):
                blocks[k].append(np.asarray(val))
            for k in ("A", "B", "Q", "R", "M", "r", "P"):
                blocks[k].append(L[k])
        out[f"{tag}/u0"] = u0s
        out[f"{tag}/x0"] = x0s
        for k, vals in blocks.items():
            out[f"{tag}/{k}"] = np.stack(vals)
    return out


# golden_v3: whole interior-point solves of the shapes at which the persistent solver's schedules
# engage (tests/test_schedules_oracle_gpu.py).  (group, family, N, pool batch, pool seed, rows, seq too)
SCHEDULE_GROUPS = [
    ("cart30", "cartpole", 30, 24, 6, 16, True),
    ("cart200", "cartpole", 200, 256, 11, 4, False),   # test_retry_repeats_accounted_bit_identical's batch
    ("pend150", "pendulum", 150, 8, 3, 4, False),      # the smallest default wide-kernel shape
]
# The row of the cart200 pool with the most KKT solves.  The index was read off a GPU solve of the
# pool (argmax of kkt_solves: 701, of them 488 accounted repeats); every value stored for it
# comes from the oracle.  None: no heavy row.
CART200_HEAVY_ROW = 112
MIN_MARGIN = 64.0


def _oracle_problem(name, N):
    return O.NumpyProblem(PR.pendulum_ocp(1.0 / N) if name == "pendulum" else PR.cartpole_ocp(1.0 / N))


def schedule_row(args):
    """One whole oracle solve (par at terminal="stage0", optionally seq) of one trajectory, with
    the margin of its closest accept test: min over the trials with a finite trial cost of
    |new_cost - cost| / (eps |cost|) -- how far the par solve stays from a decision that rounding
    could turn -- and whether it has a retry-cap run (an entry with inner > 500, P:177-182)."""
    name, N, x0, u0, seq = args
    import torch
    torch.set_num_threads(1)
    prob = _oracle_problem(name, N)
    trace = []
    U, it, solves = O.par_interior_point_optimal_control(prob, u0, x0, terminal="stage0", trace=trace)
    eps = np.finfo(np.float64).eps
    margins = [abs(t["new_cost"] - t["cost"]) / (eps * abs(t["cost"])) for t in trace
               if np.isfinite(t["new_cost"])]
    row = dict(par_u=U, par_iters=it, par_kkt_solves=solves,
               par_cost=prob.total_cost(O.rollout(prob.dynamics, U, x0), U, 0.0),
               min_margin=min(margins), retry_cap=any(t["inner"] > 500 for t in trace),
               rejected=sum(not t["success"] for t in trace))
    if seq:
        row["seq_u"], row["seq_iters"] = O.seq_interior_point_optimal_control(prob, u0, x0)
    return row


def schedule_fixtures(groups=None, heavy_row=CART200_HEAVY_ROW, workers=None):
    """golden_v3.  A row of a group's seeded pool enters only if its min_margin >= MIN_MARGIN (the
    next row of the same draw replaces it; at most half of the pool may be skipped), so that two
    correct solvers cannot disagree on it through rounding; the heavy cart200 row is exempt (its
    retry-cap run consists of sub-ulp trials by construction) and enters only with such a run."""
    import multiprocessing as mp
    sys.path.insert(0, os.path.join(ROOT, "ip-parallel-optimal-control_amd"))
    from noc import problems  # the batches the GPU tests draw (numpy only)
    out = {}
    workers = workers or min(16, os.cpu_count() or 4)
    with mp.get_context("spawn").Pool(workers) as pool:
        for tag, name, N, batch, seed, K, seq in SCHEDULE_GROUPS:
            if groups is not None and tag not in groups:
                continue
            x0s, u0s = problems.initial_conditions(name, N, batch, seed=seed)
            heavy = heavy_row if tag == "cart200" else None
            pending = None
            if heavy is not None:  # the long one first, beside the others
                pending = pool.apply_async(schedule_row, ((name, N, x0s[heavy], u0s[heavy], False),))
            rows, kept, skipped, nxt = [], [], [], 0
            while len(kept) < K:
                cand = [b for b in range(nxt, batch) if b != heavy][:K - len(kept)]
                assert cand, f"{tag}: pool exhausted"
                nxt = cand[-1] + 1
                res = pool.map(schedule_row, [(name, N, x0s[b], u0s[b], seq) for b in cand])
                for b, r in zip(cand, res):
                    ok = r["min_margin"] >= MIN_MARGIN
                    print(f"{tag} row {b}: iters {r['par_iters']} kkt_solves {r['par_kkt_solves']} "
                          f"rejected {r['rejected']} retry_cap {r['retry_cap']} "
                          f"min_margin {r['min_margin']:.1f}{'' if ok else '  SKIPPED'}", flush=True)
                    if ok:
                        kept.append(b)
                        rows.append(r)
                    else:
                        skipped.append(b)
                assert 2 * len(skipped) <= batch, f"{tag}: more than half of the pool skipped"
            heavy_in = -1
            if pending is not None:
                r = pending.get()
                print(f"{tag} heavy row {heavy}: iters {r['par_iters']} kkt_solves "
                      f"{r['par_kkt_solves']} rejected {r['rejected']} retry_cap {r['retry_cap']} "
                      f"min_margin {r['min_margin']:.3f} (exempt)"
                      f"{'' if r['retry_cap'] else '  LEFT OUT: no retry-cap run'}", flush=True)
                if r["retry_cap"]:
                    heavy_in = heavy
                    kept.append(heavy)
                    rows.append(r)
            print(f"{tag}: rows {kept} skipped {skipped}", flush=True)
            out[f"{tag}/rows"] = np.array(kept)
            out[f"{tag}/x0"] = x0s[kept]
            out[f"{tag}/u0"] = u0s[kept]
            if tag == "cart200":
                out[f"{tag}/heavy_row"] = np.array(heavy_in)
            keys = ["par_u", "par_iters", "par_kkt_solves", "par_cost", "min_margin"]
            for k in keys + (["seq_u", "seq_iters"] if seq else []):
                out[f"{tag}/{k}"] = np.stack([np.asarray(r[k]) for r in rows])
    return out


def write_v3():
    data3 = schedule_fixtures()
    path3 = os.path.join(HERE, "golden_v3.npz")
    np.savez_compressed(path3, **data3)
    print("wrote", path3, os.path.getsize(path3), "bytes,", len(data3), "arrays")


if __name__ == "__main__":
    if "--v3-only" in sys.argv:
        write_v3()
        sys.exit(0)
    data = {}
    data.update(lq_fixtures())
    data.update(ipm_fixtures())
    path = os.path.join(HERE, "golden_v1.npz")
    if "--v2-only" not in sys.argv:
        np.savez_compressed(path, **data)
        print("wrote", path, os.path.getsize(path), "bytes,", len(data), "arrays")
    data2 = newton_block_fixtures()
    path2 = os.path.join(HERE, "golden_v2.npz")
    np.savez_compressed(path2, **data2)
    print("wrote", path2, os.path.getsize(path2), "bytes,", len(data2), "arrays")
    if "--v2-only" not in sys.argv:
        write_v3()
