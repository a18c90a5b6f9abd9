// Interior-point Newton loop kernels for the registered problem families (fp64, gfx950).
//
// One host iteration of the batched driver (noc/par_interior_point_newton.py of this package)
// launches, each masked by the per-trajectory phase so every trajectory follows its own
// reference control flow (vmap semantics of the reference's nested while_loops):
//   rollout   (phase ROLLOUT)   noc/utils.py:57-63, at the start of each barrier stage (P:133)
//   linearize (phase LINEARIZE) derivatives of P:13-28 at (x_k, u_k): A=fx, B=fu, cx, cu, l_k
//   costate   (phase LINEARIZE) lambda scan C:43-54 + ru = cu + fu' lambda (P:34), total cost
//                               (P:142), |Hu|inf (P:158), ||cu||_F (P:116), terminal Hessian
//   assemble  (phase LINEARIZE) Q, R, M of compute_lqr_params (P:31-42)
//   [kkt_scan (phase SOLVE)     par_Newton's solve, P:119-123]
//   trial     (phase SOLVE)     trial point, feasibility, then the accept rule and barrier
//                               schedule of every solver (ipm_schedule.h; P:156-254, seq S:121-202)
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/noc_hip.h"
#include "block_struct.h"
#include "ipm_family.h"
#include "ipm_schedule.h"
#include "noc_internal.h"
#include "small_linalg.h"

namespace noc {

// Rollout x_{k+1} = f(x_k, u_k) (noc/utils.py:57-63), one wave64 per trajectory.  The recurrence
// is inherently sequential; every lane evaluates it redundantly (free in SIMD) with u_k broadcast
// from registers (v_readlane), so the dependent chain never waits on memory: controls are read and
// states written 64 stages at a time, coalesced.
// take_pending: also roll out trajectories the last trial marked ROLLOUT_PENDING (the
// single-stream loop, where nothing else runs concurrently).  The two-stream loop passes 0: its
// rollout runs beside the main stream's trial kernel, which may mark a trajectory (after writing
// its new u) at any moment; only the main stream's promote, ordered after that trial, turns the
// mark into ROLLOUT, so this kernel sees exactly the trajectories marked before it was launched.
template <int KIND, int NX, int NU>
__global__ __launch_bounds__(256) void rollout_kernel(noc_family prm, noc_ipm_ws w, int take_pending) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (b >= w.Bt) return;
  const int ph = w.phase[b];
  if (!(ph == NOC_PHASE_ROLLOUT || (take_pending && ph == NOC_PHASE_ROLLOUT_PENDING))) return;  // uniform per wave
  Fam<KIND, NX, NU> f(prm);
  const int N = w.N;
  double x[NX];
  NOC_UNROLL for (int i = 0; i < NX; ++i) x[i] = w.x0[(size_t)b * NX + i];
  double* X = w.x + (size_t)b * (N + 1) * NX;
  const double* U = w.u + (size_t)b * N * NU;
  if (lane < NX) X[lane] = x[lane];
  for (int base = 0; base < N; base += 64) {
    const int k = base + lane;
    double uk[NU];
    NOC_UNROLL for (int j = 0; j < NU; ++j) uk[j] = (k < N) ? U[(size_t)k * NU + j] : 0.0;
    double mine[NX];
    NOC_UNROLL for (int i = 0; i < NX; ++i) mine[i] = 0.0;
    const int cnt = (N - base < 64) ? (N - base) : 64;
    for (int t = 0; t < cnt; ++t) {
      double ut[NU], xn[NX];
      NOC_UNROLL for (int j = 0; j < NU; ++j) ut[j] = readlane_d(uk[j], t);
      f.step(x, ut, xn);
      NOC_UNROLL for (int i = 0; i < NX; ++i) {
        x[i] = xn[i];
        mine[i] = (lane == t) ? xn[i] : mine[i];
      }
    }
    if (k < N) NOC_UNROLL for (int i = 0; i < NX; ++i) X[(size_t)(k + 1) * NX + i] = mine[i];
  }
  if (lane == 0) w.phase[b] = NOC_PHASE_ROLLED;
}

// ROLLED -> LINEARIZE; ROLLOUT_PENDING -> ROLLOUT (the next step's rollout picks it up)
__global__ __launch_bounds__(256) void promote_kernel(noc_ipm_ws w) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= w.Bt) return;
  const int ph = w.phase[b];
  if (ph == NOC_PHASE_ROLLED) w.phase[b] = NOC_PHASE_LINEARIZE;
  else if (ph == NOC_PHASE_ROLLOUT_PENDING) w.phase[b] = NOC_PHASE_ROLLOUT;
}

// thread per (trajectory, chunk slot, lane) in tiled order: the A/B stores are coalesced
// COMPACT (here and in the costate / assemble kernels): w.A, w.B, w.Q, w.R, w.M are the compact
// tiled fields (block_struct.h: the variable entries only, the layout noc_ipm_solve keeps there);
// the constants are rebuilt where a block is read -- the same doubles the dense fields hold
template <int KIND, int NX, int NU, bool COMPACT>
__global__ __launch_bounds__(256) void linearize_kernel(noc_family prm, noc_ipm_ws w) {
#include "ipm_body_linearize.h"
}
// per-trajectory cost parameters (noc_ipm_prepare_params): the same body, dense blocks, on a
// family argument that first takes trajectory b's goal, wx, wu, wf, u_bound from its record in tp
template <int KIND, int NX, int NU>
__global__ __launch_bounds__(256) void linearize_params_kernel(noc_family prm, noc_ipm_ws w,
                                                              const double* __restrict__ tp) {
  constexpr bool COMPACT = false;
  {
    const long long tt = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long per = (long long)((w.N + w.lanes - 1) / w.lanes) * w.lanes;
    if (tt >= (long long)w.Bt * per) return;  // as the body
    load_traj_params<NX, NU>(prm, tp, (int)(tt / per));
  }
#include "ipm_body_linearize.h"
}

// Costates as a reverse affine scan over the horizon (the par_costates pattern, C:34-40),
// one L-lane segment per trajectory with the KKT scan's chunk geometry (tiled A, B, cx, cu, lc):
//   lambda_k = cx_k + A_k' lambda_{k+1},  lambda_N = grad final_cost (C:44-52)
// plus, per trajectory: ru_k = cu_k + B_k' lambda_{k+1} (P:34, tiled), total cost (P:142),
// max|ru| (P:158), ||cu||_F (P:116), the regularisation fed to the KKT solve and the terminal
// Hessian hessian(final_cost) (S:66).
template <int KIND, int NX, int NU, int L, bool COMPACT>
__global__ __launch_bounds__(64) void costate_scan_kernel(noc_family prm, noc_ipm_ws w, int mode) {
#include "ipm_body_costate.h"
}
// per-trajectory cost parameters: as linearize_params_kernel
template <int KIND, int NX, int NU, int L>
__global__ __launch_bounds__(64) void costate_scan_params_kernel(noc_family prm, noc_ipm_ws w, int mode,
                                                                const double* __restrict__ tp) {
  constexpr bool COMPACT = false;
  {
    const int bt = (int)((blockIdx.x * blockDim.x + threadIdx.x) / L);
    if (bt >= w.Bt) return;  // as the body
    load_traj_params<NX, NU>(prm, tp, bt);
  }
#include "ipm_body_costate.h"
}


template <int KIND, int NX, int NU>
static void launch_costate_params(const noc_family& p, const noc_ipm_ws& w, int mode, const double* tp,
                                  hipStream_t s) {
  const int L = w.lanes;
  const unsigned grid = (unsigned)(((long long)w.Bt * L + 63) / 64);
  switch (L) {
    case 64: hipLaunchKernelGGL((costate_scan_params_kernel<KIND, NX, NU, 64>), dim3(grid), dim3(64), 0, s, p, w, mode, tp); break;
    case 32: hipLaunchKernelGGL((costate_scan_params_kernel<KIND, NX, NU, 32>), dim3(grid), dim3(64), 0, s, p, w, mode, tp); break;
    case 16: hipLaunchKernelGGL((costate_scan_params_kernel<KIND, NX, NU, 16>), dim3(grid), dim3(64), 0, s, p, w, mode, tp); break;
    case 8: hipLaunchKernelGGL((costate_scan_params_kernel<KIND, NX, NU, 8>), dim3(grid), dim3(64), 0, s, p, w, mode, tp); break;
    default: hipLaunchKernelGGL((costate_scan_params_kernel<KIND, NX, NU, 1>), dim3(grid), dim3(64), 0, s, p, w, mode, tp); break;
  }
}

template <int KIND, int NX, int NU, bool COMPACT>
static void launch_costate(const noc_family& p, const noc_ipm_ws& w, int mode, hipStream_t s) {
  const int L = w.lanes;
  const unsigned grid = (unsigned)(((long long)w.Bt * L + 63) / 64);
  switch (L) {
    case 64: hipLaunchKernelGGL((costate_scan_kernel<KIND, NX, NU, 64, COMPACT>), dim3(grid), dim3(64), 0, s, p, w, mode); break;
    case 32: hipLaunchKernelGGL((costate_scan_kernel<KIND, NX, NU, 32, COMPACT>), dim3(grid), dim3(64), 0, s, p, w, mode); break;
    case 16: hipLaunchKernelGGL((costate_scan_kernel<KIND, NX, NU, 16, COMPACT>), dim3(grid), dim3(64), 0, s, p, w, mode); break;
    case 8: hipLaunchKernelGGL((costate_scan_kernel<KIND, NX, NU, 8, COMPACT>), dim3(grid), dim3(64), 0, s, p, w, mode); break;
    default: hipLaunchKernelGGL((costate_scan_kernel<KIND, NX, NU, 1, COMPACT>), dim3(grid), dim3(64), 0, s, p, w, mode); break;
  }
}

template <int KIND, int NX, int NU, bool COMPACT>
__global__ __launch_bounds__(256) void assemble_kernel(noc_family prm, noc_ipm_ws w, int terminal) {
#include "ipm_body_assemble.h"
}
// per-trajectory cost parameters: as linearize_params_kernel
template <int KIND, int NX, int NU>
__global__ __launch_bounds__(256) void assemble_params_kernel(noc_family prm, noc_ipm_ws w, int terminal,
                                                             const double* __restrict__ tp) {
  constexpr bool COMPACT = false;
  {
    const long long tt = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long per = (long long)((w.N + w.lanes - 1) / w.lanes) * w.lanes;
    if (tt >= (long long)w.Bt * per) return;  // as the body
    load_traj_params<NX, NU>(prm, tp, (int)(tt / per));
  }
#include "ipm_body_assemble.h"
}

__global__ __launch_bounds__(256) void mark_solve_kernel(noc_ipm_ws w) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= w.Bt) return;
  const int ph = w.phase[b];
  if (ph == NOC_PHASE_LINEARIZE) w.phase[b] = NOC_PHASE_SOLVE;
  w.kkt_active[b] = (ph == NOC_PHASE_LINEARIZE || ph == NOC_PHASE_SOLVE) ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------
// trial point + Newton / barrier logic: one wave64 per trajectory (4 per 256-thread block)

template <int KIND, int NX, int NU>
__global__ __launch_bounds__(256) void trial_kernel(noc_family prm, noc_ipm_ws w, int mode) {
#include "ipm_body_trial.h"
}
// per-trajectory cost parameters (noc_ipm_trial_params): as linearize_params_kernel; the
// trajectory is wave-uniform here
template <int KIND, int NX, int NU>
__global__ __launch_bounds__(256) void trial_params_kernel(noc_family prm, noc_ipm_ws w, int mode,
                                                          const double* __restrict__ tp) {
  {
    const int bt = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (bt >= w.Bt) return;  // as the body
    load_traj_params<NX, NU>(prm, tp, __builtin_amdgcn_readfirstlane(bt));
  }
#include "ipm_body_trial.h"
}

__global__ __launch_bounds__(256) void init_kernel(noc_ipm_ws w, double bp0) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= w.Bt) return;
  w.phase[b] = NOC_PHASE_ROLLOUT;
  w.kkt_active[b] = 1;
  w.it[b] = 0;
  w.inner[b] = 0;
  w.total_it[b] = 0;
  w.kkt_solves[b] = 0;
  if (w.repeats) w.repeats[b] = 0;
  w.bp[b] = bp0;
  w.rp[b] = 1.0;
  w.rinc[b] = 2.0;
  w.hu[b] = 1.0;
}

// ------------------------------------------------------------------------------------------------
template <int KIND, int NX, int NU>
static hipError_t rollout_t(const noc_family& p, const noc_ipm_ws& w, hipStream_t s,
                           int take_pending) {
  hipLaunchKernelGGL((rollout_kernel<KIND, NX, NU>), dim3((w.Bt + 3) / 4), dim3(256), 0, s, p, w,
                     take_pending);
  return hipGetLastError();
}

// linearise + costates + LQ blocks for phase-LINEARIZE trajectories, then LINEARIZE -> SOLVE
template <int KIND, int NX, int NU, bool COMPACT>
static hipError_t prepare_main_c(const noc_family& p, const noc_ipm_ws& w, int mode, int terminal,
                                 hipStream_t s) {
  const int bt_grid = (w.Bt + 255) / 256;
  const long long cmax = (w.N + w.lanes - 1) / w.lanes;
  const unsigned st_grid = (unsigned)(((long long)w.Bt * cmax * w.lanes + 255) / 256);
  hipLaunchKernelGGL((linearize_kernel<KIND, NX, NU, COMPACT>), dim3(st_grid), dim3(256), 0, s, p, w);
  launch_costate<KIND, NX, NU, COMPACT>(p, w, mode, s);
  hipLaunchKernelGGL((assemble_kernel<KIND, NX, NU, COMPACT>), dim3(st_grid), dim3(256), 0, s, p, w, terminal);
  hipLaunchKernelGGL(mark_solve_kernel, dim3(bt_grid), dim3(256), 0, s, w);
  return hipGetLastError();
}

// compact: the workspace's block fields are the compact ones (the _compact entry points)
template <int KIND, int NX, int NU>
static hipError_t prepare_main_t(const noc_family& p, const noc_ipm_ws& w, int mode, int terminal,
                                 bool compact, hipStream_t s) {
  return compact ? prepare_main_c<KIND, NX, NU, true>(p, w, mode, terminal, s)
                 : prepare_main_c<KIND, NX, NU, false>(p, w, mode, terminal, s);
}

template <int KIND, int NX, int NU>
static hipError_t prepare_t(const noc_family& p, const noc_ipm_ws& w, int mode, int terminal,
                            bool compact, hipStream_t s) {
  hipError_t e = rollout_t<KIND, NX, NU>(p, w, s, 1);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(promote_kernel, dim3((w.Bt + 255) / 256), dim3(256), 0, s, w);
  return prepare_main_t<KIND, NX, NU>(p, w, mode, terminal, compact, s);
}

template <int KIND, int NX, int NU>
static hipError_t trial_t(const noc_family& p, const noc_ipm_ws& w, int mode, hipStream_t s) {
  const unsigned grid = (unsigned)((w.Bt + 3) / 4);
  hipLaunchKernelGGL((trial_kernel<KIND, NX, NU>), dim3(grid), dim3(256), 0, s, p, w, mode);
  return hipGetLastError();
}

// family dispatch: one instantiation per NOC_FAMILY line of families.def
hipError_t ipm_prepare(const noc_family& p, const noc_ipm_ws& w, int mode, int terminal,
                       bool compact, hipStream_t s) {
#define NOC_FAMILY(K, X, U) \
  if (p.kind == K && p.nx == X && p.nu == U) return prepare_t<K, X, U>(p, w, mode, terminal, compact, s);
#include NOC_FAMILIES_DEF
#undef NOC_FAMILY
  return hipErrorInvalidValue;
}

hipError_t ipm_rollout(const noc_family& p, const noc_ipm_ws& w, hipStream_t s) {
#define NOC_FAMILY(K, X, U) \
  if (p.kind == K && p.nx == X && p.nu == U) return rollout_t<K, X, U>(p, w, s, 0);
#include NOC_FAMILIES_DEF
#undef NOC_FAMILY
  return hipErrorInvalidValue;
}

hipError_t ipm_prepare_main(const noc_family& p, const noc_ipm_ws& w, int mode, int terminal,
                            bool compact, hipStream_t s) {
#define NOC_FAMILY(K, X, U) \
  if (p.kind == K && p.nx == X && p.nu == U) return prepare_main_t<K, X, U>(p, w, mode, terminal, compact, s);
#include NOC_FAMILIES_DEF
#undef NOC_FAMILY
  return hipErrorInvalidValue;
}

hipError_t ipm_promote(const noc_ipm_ws& w, hipStream_t s) {
  hipLaunchKernelGGL(promote_kernel, dim3((w.Bt + 255) / 256), dim3(256), 0, s, w);
  return hipGetLastError();
}

hipError_t ipm_trial(const noc_family& p, const noc_ipm_ws& w, int mode, hipStream_t s) {
#define NOC_FAMILY(K, X, U) \
  if (p.kind == K && p.nx == X && p.nu == U) return trial_t<K, X, U>(p, w, mode, s);
#include NOC_FAMILIES_DEF
#undef NOC_FAMILY
  return hipErrorInvalidValue;
}

// ---- per-trajectory cost parameters: the params forms of prepare and trial (the rollout needs
// none: it reads dt and the dynamics only).  Dense blocks.
template <int KIND, int NX, int NU>
constexpr bool traj_params_instance() { return !Fam<KIND, NX, NU>::kGenCost; }

template <int KIND, int NX, int NU>
static hipError_t prepare_params_t(const noc_family& p, const noc_ipm_ws& w, const double* tp, int mode,
                                   int terminal, hipStream_t s) {
  if constexpr (traj_params_instance<KIND, NX, NU>()) {
    hipError_t e = rollout_t<KIND, NX, NU>(p, w, s, 1);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(promote_kernel, dim3((w.Bt + 255) / 256), dim3(256), 0, s, w);
    const int bt_grid = (w.Bt + 255) / 256;
    const long long cmax = (w.N + w.lanes - 1) / w.lanes;
    const unsigned st_grid = (unsigned)(((long long)w.Bt * cmax * w.lanes + 255) / 256);
    hipLaunchKernelGGL((linearize_params_kernel<KIND, NX, NU>), dim3(st_grid), dim3(256), 0, s, p, w, tp);
    launch_costate_params<KIND, NX, NU>(p, w, mode, tp, s);
    hipLaunchKernelGGL((assemble_params_kernel<KIND, NX, NU>), dim3(st_grid), dim3(256), 0, s, p, w, terminal, tp);
    hipLaunchKernelGGL(mark_solve_kernel, dim3(bt_grid), dim3(256), 0, s, w);
    return hipGetLastError();
  } else {
    return hipErrorInvalidValue;
  }
}

template <int KIND, int NX, int NU>
static hipError_t trial_params_t(const noc_family& p, const noc_ipm_ws& w, const double* tp, int mode,
                                 hipStream_t s) {
  if constexpr (traj_params_instance<KIND, NX, NU>()) {
    hipLaunchKernelGGL((trial_params_kernel<KIND, NX, NU>), dim3((unsigned)((w.Bt + 3) / 4)), dim3(256), 0, s, p,
                       w, mode, tp);
    return hipGetLastError();
  } else {
    return hipErrorInvalidValue;
  }
}

hipError_t ipm_prepare_params(const noc_family& p, const noc_ipm_ws& w, const double* tp, int mode,
                              int terminal, hipStream_t s) {
#define NOC_FAMILY(K, X, U) \
  if (p.kind == K && p.nx == X && p.nu == U) return prepare_params_t<K, X, U>(p, w, tp, mode, terminal, s);
#include NOC_FAMILIES_DEF
#undef NOC_FAMILY
  return hipErrorInvalidValue;
}

hipError_t ipm_trial_params(const noc_family& p, const noc_ipm_ws& w, const double* tp, int mode,
                            hipStream_t s) {
#define NOC_FAMILY(K, X, U) \
  if (p.kind == K && p.nx == X && p.nu == U) return trial_params_t<K, X, U>(p, w, tp, mode, s);
#include NOC_FAMILIES_DEF
#undef NOC_FAMILY
  return hipErrorInvalidValue;
}

// a family with the parametrised quadratic cost (not a registered family's traced costs)
bool traj_params_supported(const noc_family& p) {
#define NOC_FAMILY(K, X, U) \
  if (p.kind == K && p.nx == X && p.nu == U) return traj_params_instance<K, X, U>();
#include NOC_FAMILIES_DEF
#undef NOC_FAMILY
  return false;
}

hipError_t ipm_init(const noc_ipm_ws& w, double bp0, hipStream_t s) {
  hipLaunchKernelGGL(init_kernel, dim3((w.Bt + 255) / 256), dim3(256), 0, s, w, bp0);
  return hipGetLastError();
}

bool family_supported(const noc_family& p) {
#define NOC_FAMILY(K, X, U) \
  if (p.kind == K && p.nx == X && p.nu == U) return true;
#include NOC_FAMILIES_DEF
#undef NOC_FAMILY
  return false;
}

}  // namespace noc
