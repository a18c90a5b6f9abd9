"""Cost of per-trajectory parameters on the flagship shape: cart-pole N = 200, Bt = 4096 through
the shared-parameter persistent solve and through the params solve with uniform rows (every
trajectory repeats the family's own goal / weights / bound), both schedule="index", same build,
same process.

Protocol: both engines are built and warmed up first (code objects loaded, every shape launched),
then the two solves alternate for --repeats rounds, each timed with device events around one whole
solve (tens of milliseconds of device work); the outputs of the two are compared bit for bit at the
timed size.  Prints one JSON line: the medians, the min-max spread of each, and their ratio.

    python tools/traj_params_bench.py [--N 200] [--batch 4096] [--repeats 9] [--warmup 2]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ip-parallel-optimal-control_amd"))

import noc  # noqa: E402
from noc import problems  # noqa: E402
from noc.ipm import BatchedIPM  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=200)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    ocp = problems.make_problem("cartpole", a.N)
    fam = ocp.family
    x0, u0 = problems.initial_conditions("cartpole", a.N, a.batch, seed=0)
    uniform = noc.TrajectoryParams(goal=fam.goal, wx=fam.wx, wu=fam.wu, wf=fam.wf,
                                   u_bound=np.full(a.batch, fam.u_bound))
    engines = {}
    for key, prm in (("shared", None), ("params", uniform)):
        eng = BatchedIPM(fam, a.N, a.batch, persistent=True)
        eng.load_params(prm)
        engines[key] = eng

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
        for key in engines:  # alternating, so drift of the machine hits both alike
            times[key].append(run(key))
    same = all(torch.equal(engines["shared"].t[k], engines["params"].t[k])
               for k in ("u", "x", "total_it", "kkt_solves", "cost"))
    med = {k: float(np.median(v)) for k, v in times.items()}
    out = dict(workload=f"cartpole N={a.N} Bt={a.batch} persistent schedule=index",
               repeats=a.repeats, warmup=a.warmup,
               shared_ms=med["shared"], shared_min_max_ms=[min(times["shared"]), max(times["shared"])],
               params_ms=med["params"], params_min_max_ms=[min(times["params"]), max(times["params"])],
               ratio_params_over_shared=med["params"] / med["shared"], outputs_bit_identical=same)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
