"""Cost of per-trajectory parameters in one-launch interior-point DDP: cart-pole N = 200 through
noc_ddp_solve_ex (shared parameters) and through noc_ddp_solve_params with uniform rows (every
trajectory repeats the family's own goal / weights / bound), same build, same process.

Protocol (after tools/traj_params_bench.py): inputs, workspace and records live on the device;
both entry points are warmed up first (code objects loaded), then the two solves alternate for
--repeats rounds, each timed with device events around one whole solve (the controls are restored
from a device copy before the first event); the outputs of the two are compared bit for bit.
--batch defaults to one trajectory per SIMD of an MI355X (1024 waves: one solve takes some hundred
milliseconds, 266 ms when measured).  Prints one JSON line: the medians, the min-max spread of each, and their ratio -- the
shared side's own spread is the yardstick for the ratio.

    python tools/ddp_params_bench.py [--N 200] [--batch 1024] [--repeats 9] [--warmup 2]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ip-parallel-optimal-control_amd"))

import noc  # noqa: E402
from noc import _lib, problems  # noqa: E402
from noc.traj_params import pack  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=200)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    N, Bt = a.N, a.batch
    ocp = problems.make_problem("cartpole", N)
    fam = ocp.family
    famc = fam.to_c()
    lib = _lib.load_for(fam)
    x0, u0 = problems.initial_conditions("cartpole", N, Bt, seed=0)
    uniform = noc.TrajectoryParams(goal=fam.goal, wx=fam.wx, wu=fam.wu, wf=fam.wf,
                                   u_bound=np.full(Bt, fam.u_bound))
    dev = torch.device("cuda")
    f64 = dict(device=dev, dtype=torch.float64)
    i32 = dict(device=dev, dtype=torch.int32)
    X0, U0 = torch.as_tensor(x0, **f64).contiguous(), torch.as_tensor(u0, **f64).contiguous()
    rec = torch.as_tensor(pack(uniform, fam, Bt), **f64).contiguous()
    st = {}
    for key in ("shared", "params"):
        st[key] = dict(U=torch.empty_like(U0),
                       work=torch.empty(int(lib.noc_ddp_work_doubles(fam.nx, fam.nu, N, Bt)), **f64),
                       its=torch.zeros(Bt, **i32), passes=torch.zeros(Bt, **i32),
                       done=torch.zeros(Bt, **i32))

    def run(key):
        s = st[key]
        s["U"].copy_(U0)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        head = (ctypes.byref(famc), N, Bt, X0.data_ptr(), s["U"].data_ptr(), s["work"].data_ptr(),
                s["its"].data_ptr(), s["passes"].data_ptr(), s["done"].data_ptr())
        t0.record()
        if key == "params":
            rc = lib.noc_ddp_solve_params(*head, rec.data_ptr(), 0.1, 10 ** 7, 0,
                                          _lib.stream_handle(dev))
        else:
            rc = lib.noc_ddp_solve_ex(*head, 0.1, 10 ** 7, 0, _lib.stream_handle(dev))
        t1.record()
        _lib.check(rc, "noc_ddp_solve" + ("_params" if key == "params" else "_ex"), lib)
        torch.cuda.synchronize()
        return t0.elapsed_time(t1)

    for _ in range(a.warmup):
        for key in st:
            run(key)
    times = {k: [] for k in st}
    for _ in range(a.repeats):
        for key in st:  # alternating, so drift of the machine hits both alike
            times[key].append(run(key))
    nX = Bt * (N + 1) * fam.nx
    same = all(torch.equal(st["shared"][k], st["params"][k]) for k in ("U", "its", "passes", "done")) \
        and torch.equal(st["shared"]["work"][:nX], st["params"]["work"][:nX])
    med = {k: float(np.median(v)) for k, v in times.items()}
    out = dict(workload=f"cartpole N={N} Bt={Bt} one-launch DDP",
               repeats=a.repeats, warmup=a.warmup,
               shared_ms=med["shared"], shared_min_max_ms=[min(times["shared"]), max(times["shared"])],
               params_ms=med["params"], params_min_max_ms=[min(times["params"]), max(times["params"])],
               ratio_params_over_shared=med["params"] / med["shared"],
               shared_spread_max_over_min=max(times["shared"]) / min(times["shared"]),
               all_done=bool(st["params"]["done"].bool().all()), outputs_bit_identical=same)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
