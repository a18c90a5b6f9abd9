"""Cost of RK4 stages: one whole cart-pole solve, N = 200, Bt = 4096, through the persistent solver
for the RK4 family of tests/integrator_families.py against the Euler family of the same ODE and
cost (dt = 0.05), same process.

Protocol (as tools/traj_params_bench.py): every engine is built and warmed up first, then the
solves alternate for --repeats rounds, each timed with device events around one whole solve.  The
two families solve different discrete problems, so their Newton iterations and KKT solves are
reported next to the times and the time per KKT solve is the comparable figure.

--extra NAME=PATH adds the RK4 family loaded from another build of its library (e.g. one compiled
without -DNOC_SCAN_CONTRACT_ON, to separate the scan's contraction from the derivative work).
Build the families before a GPU run.  Prints one JSON line.

    python tools/integrator_bench.py [--N 200] [--batch 4096] [--repeats 7] [--warmup 2]
"""
import argparse
import dataclasses
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ip-parallel-optimal-control_amd"), os.path.join(ROOT, "tests")]

import integrator_families as IF  # noqa: E402
from noc import _lib, problems  # noqa: E402
from noc.ipm import BatchedIPM  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=200)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--extra", action="append", default=[])
    a = ap.parse_args()
    fams = {"euler": IF.register("rk4_cartpole", integrator="euler").family,
            "rk4": IF.register("rk4_cartpole").family}
    for item in a.extra:
        key, path = item.split("=", 1)
        fams[key] = dataclasses.replace(fams["rk4"], lib_path=os.path.abspath(path))
    x0, u0 = problems.initial_conditions("cartpole", a.N, a.batch, seed=0)
    engines = {k: BatchedIPM(f, a.N, a.batch, persistent=True) for k, f in fams.items()}

    def run(key):
        eng = engines[key]
        eng.load(u0, x0)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        eng.solve_persistent(schedule="index")
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1)

    for _ in range(a.warmup):
        for key in engines:
            run(key)
    times = {k: [] for k in engines}
    for _ in range(a.repeats):
        for key in engines:  # alternating, so drift of the machine hits all alike
            times[key].append(run(key))
    out = dict(workload=f"cartpole ODE dt={IF.DT} N={a.N} Bt={a.batch} persistent schedule=index",
               repeats=a.repeats, warmup=a.warmup)
    for k, eng in engines.items():
        _, it, s = eng.result()
        ms, solves = float(np.median(times[k])), int(s.sum().item())
        out[k] = dict(ms=ms, min_max_ms=[min(times[k]), max(times[k])], iterations=int(it.sum().item()),
                      kkt_solves=solves, us_per_1000_kkt_solves=1e6 * ms / solves,
                      done=bool((eng.t["phase"] == _lib.PHASE_DONE).all().item()))
    out["ratio_rk4_over_euler_per_solve"] = (out["rk4"]["us_per_1000_kkt_solves"]
                                             / out["euler"]["us_per_1000_kkt_solves"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
