"""Per-trajectory cost parameters of a batched solve (include/noc_hip.h: NOC_TRAJ_PARAM_DOUBLES).

A heterogeneous batch solves trajectory b with its own goal, wx, wu, wf and u_bound; dt,
wrap_index, the linear family's A, B and the dynamics stay the family's.  TrajectoryParams names
the fields a caller varies; pack() turns it, against a Family, into the (Bt, 32) record the
noc_*_params entry points read.  Pure numpy: no device and no library are needed to pack
(device_records puts a packed record on the device for the building blocks).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

PARAM_DOUBLES = 32  # NOC_TRAJ_PARAM_DOUBLES
# NOC_TP_*: offset and capacity of each field of a record
_OFF = dict(goal=(0, 8), wx=(8, 8), wu=(16, 4), wf=(20, 8))
_UBOUND = 28


@dataclass
class TrajectoryParams:
    """Each of goal, wx, wf (n = nx) and wu (n = nu) is None (the family's value for every
    trajectory), shape (n,) (one value for every trajectory) or shape (Bt, n) (row b for
    trajectory b); u_bound is None, a scalar or shape (Bt,)."""
    goal: Optional[object] = None
    wx: Optional[object] = None
    wu: Optional[object] = None
    wf: Optional[object] = None
    u_bound: Optional[object] = None

    def rows(self, lo: int, hi: int) -> "TrajectoryParams":
        """The parameters of trajectories lo .. hi-1 (per-trajectory fields sliced, shared ones
        kept): what a shard of the batch is solved with (noc.distributed.solve_sharded)."""
        def cut(v, per_row_ndim):
            if v is None:
                return None
            a = np.asarray(v, dtype=np.float64)
            return a[lo:hi] if a.ndim == per_row_ndim else a
        return TrajectoryParams(goal=cut(self.goal, 2), wx=cut(self.wx, 2), wu=cut(self.wu, 2),
                                wf=cut(self.wf, 2), u_bound=cut(self.u_bound, 1))


def pack(params: TrajectoryParams, family, Bt: int) -> np.ndarray:
    """The (Bt, 32) fp64 record of `params` against `family`: goal[8] wx[8] wu[4] wf[8] u_bound and
    three reserved zeros per row, unspecified fields filled from the family.  ValueError on a
    wrong shape, a non-finite entry, u_bound <= 0 for a family with a bound, or a u_bound given for
    a family without one (a trajectory may move its bound, not switch the barrier on or off)."""
    if not isinstance(params, TrajectoryParams):
        raise ValueError("params must be a noc.traj_params.TrajectoryParams")
    Bt = int(Bt)
    nx, nu = int(family.nx), int(family.nu)
    rec = np.zeros((Bt, PARAM_DOUBLES), dtype=np.float64)
    for name, n in (("goal", nx), ("wx", nx), ("wu", nu), ("wf", nx)):
        off, _cap = _OFF[name]
        v = getattr(params, name)
        if v is None:
            own = [float(t) for t in getattr(family, name)][:n]  # Family.to_c: missing entries are 0
            a = np.asarray(own + [0.0] * (n - len(own)), dtype=np.float64)
        else:
            a = np.asarray(v, dtype=np.float64)
        if a.shape not in ((n,), (Bt, n)):
            raise ValueError(f"TrajectoryParams.{name}: shape {a.shape}, expected ({n},) or ({Bt}, {n})")
        if not np.all(np.isfinite(a)):
            raise ValueError(f"TrajectoryParams.{name}: non-finite entry")
        rec[:, off:off + n] = a
    fam_ub = float(family.u_bound)
    if params.u_bound is None:
        rec[:, _UBOUND] = fam_ub
    else:
        ub = np.asarray(params.u_bound, dtype=np.float64)
        if ub.shape not in ((), (Bt,)):
            raise ValueError(f"TrajectoryParams.u_bound: shape {ub.shape}, expected a scalar or ({Bt},)")
        if not np.all(np.isfinite(ub)):
            raise ValueError("TrajectoryParams.u_bound: non-finite entry")
        if not fam_ub > 0.0:
            raise ValueError("TrajectoryParams.u_bound given for a family without a control bound: "
                             "a trajectory may move its bound, not switch the barrier on")
        if np.any(ub <= 0.0):
            raise ValueError("TrajectoryParams.u_bound must be > 0 for a family with a control bound")
        rec[:, _UBOUND] = ub
    return rec


def device_records(fn: str, params, family, B: int, single: bool, device):
    """The (B, 32) fp64 device tensor a noc_*_params building block reads: `params` packed against
    `family` (ValueError on a bad field), or `params` itself when it already is such a tensor (a
    loop over the blocks packs once: differential_dynamic_programming._solve_blocks).  NocError for
    an unbatched call (the record is per trajectory of a batch) or a mis-shaped record, before
    anything reaches the device."""
    import torch
    from . import _lib
    if single:
        raise _lib.NocError(f"{fn}: params needs batched inputs (a leading batch axis): one "
                            f"record per trajectory")
    if isinstance(params, torch.Tensor):
        if tuple(params.shape) != (B, PARAM_DOUBLES) or params.dtype != torch.float64:
            raise _lib.NocError(f"{fn}: a packed params record must be a ({B}, {PARAM_DOUBLES}) "
                                f"float64 tensor; got {tuple(params.shape)} {params.dtype}")
        _lib.require_device(params, "params")
        return params.contiguous()
    return torch.as_tensor(pack(params, family, B), device=device).contiguous()
