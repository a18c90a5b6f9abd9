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
// Per-trajectory cost parameters (noc_ipm_prepare_params, noc_ipm_trial_params): TP... tp is
// empty, or the records (ipm_family.h: TrajParams) -- then the family argument first takes
// trajectory b's goal, wx, wu, wf, u_bound from its record.  Those instances run on dense blocks.
template <int KIND, int NX, int NU, bool COMPACT, class... TP>
__global__ __launch_bounds__(256) void linearize_kernel(noc_family prm, noc_ipm_ws w, TP... tp) {
  if constexpr (sizeof...(TP) > 0) {  // b = t / (chunk slots x lanes) per thread: vector loads
    const long long tt = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long per = (long long)((w.N + w.lanes - 1) / w.lanes) * w.lanes;
    if (tt >= (long long)w.Bt * per) return;  // keeps the record read in range
    load_traj_params<NX, NU>(prm, tp..., (int)(tt / per));
  }
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int N = w.N, L = w.lanes;
  const Chunks ch(N, L);
  if (t >= (long long)w.Bt * ch.cmax * L) return;
  const int b = (int)(t / ((long long)ch.cmax * L));
  const int rem = (int)(t % ((long long)ch.cmax * L));
  const int j = rem / L, l = rem % L;
  if (j >= ch.len(l) || !builds_blocks(w, b)) return;
  const int k = ch.start(l) + j;
  const size_t tn = (size_t)b * N + k;
  Fam<KIND, NX, NU> f(prm);
  const double bp = w.bp[b];
  double x[NX], u[NU];
  gload<NX>(w.x + ((size_t)b * (N + 1) + k) * NX, x);
  NOC_UNROLL for (int i = 0; i < NU; ++i) u[i] = w.u[tn * NU + i];
  double fx[NX * NX], fu[NX * NU], cx[NX], cu[NU];  // all stored tiled
  f.jac(x, u, fx, fu);
  f.stage_grad(x, u, bp, cx, cu);
  if constexpr (COMPACT) {
    using BS = BlockStruct<KIND, NX, NU, true>;
    constexpr int VA = BS::template nv<BF_A>(), VB = BS::template nv<BF_B>();
    double va[VA > 0 ? VA : 1], vb[VB > 0 ? VB : 1];
    BS::template compress<BF_A>(fx, va);
    BS::template compress<BF_B>(fu, vb);
    if constexpr (VA > 0) tstore_rt<VA>(w.A, L, ch.cmax, b, j, l, va);
    if constexpr (VB > 0) tstore_rt<VB>(w.B, L, ch.cmax, b, j, l, vb);
  } else {
    tstore_rt<NX * NX>(w.A, L, ch.cmax, b, j, l, fx);
    tstore_rt<NX * NU>(w.B, L, ch.cmax, b, j, l, fu);
  }
  tstore_rt<NX>(w.cx, L, ch.cmax, b, j, l, cx);
  tstore_rt<NU>(w.cu, L, ch.cmax, b, j, l, cu);
  const double lc = f.stage_cost(x, u, bp);
  tstore_rt<1>(w.lc, L, ch.cmax, b, j, l, &lc);
}

// Costates as a reverse affine scan over the horizon (the par_costates pattern, C:34-40),
// one L-lane segment per trajectory with the KKT scan's chunk geometry (tiled A, B, cx, cu, lc):
//   lambda_k = cx_k + A_k' lambda_{k+1},  lambda_N = grad final_cost (C:44-52)
// plus, per trajectory: ru_k = cu_k + B_k' lambda_{k+1} (P:34, tiled), total cost (P:142),
// max|ru| (P:158), ||cu||_F (P:116), the regularisation fed to the KKT solve and the terminal
// Hessian hessian(final_cost) (S:66).
// (This kernel keeps a twin for the per-trajectory records, and the two share their body through
// ipm_body_costate.h, included between their braces: folded into one kernel like the others, by a
// trailing argument pack or by a force-inlined body function, the (8, 4) instances' register
// allocation moved -- profiles/r10/params_fold/README.md.)
template <int KIND, int NX, int NU, int L, bool COMPACT>
__global__ __launch_bounds__(64) void costate_scan_kernel(noc_family prm, noc_ipm_ws w, int mode) {
#include "ipm_body_costate.h"
}
// per-trajectory cost parameters: b per L-lane segment, vector loads; dense blocks
template <int KIND, int NX, int NU, int L>
__global__ __launch_bounds__(64) void costate_scan_params_kernel(noc_family prm, noc_ipm_ws w, int mode,
                                                                const double* __restrict__ tp) {
  constexpr bool COMPACT = false;
  {
    const int bt = (int)((blockIdx.x * blockDim.x + threadIdx.x) / L);
    if (bt >= w.Bt) return;  // as the body: keeps the record read in range
    load_traj_params<NX, NU>(prm, tp, bt);
  }
#include "ipm_body_costate.h"
}

template <int KIND, int NX, int NU, int L, bool COMPACT, class... TP>
static void launch_costate_l(const noc_family& p, const noc_ipm_ws& w, int mode, unsigned grid, hipStream_t s,
                             TP... tp) {
  if constexpr (sizeof...(TP) > 0)
    hipLaunchKernelGGL((costate_scan_params_kernel<KIND, NX, NU, L>), dim3(grid), dim3(64), 0, s, p, w, mode, tp...);
  else
    hipLaunchKernelGGL((costate_scan_kernel<KIND, NX, NU, L, COMPACT>), dim3(grid), dim3(64), 0, s, p, w, mode);
}

template <int KIND, int NX, int NU, bool COMPACT, class... TP>
static void launch_costate(const noc_family& p, const noc_ipm_ws& w, int mode, hipStream_t s, TP... tp) {
  const int L = w.lanes;
  const unsigned grid = (unsigned)(((long long)w.Bt * L + 63) / 64);
  switch (L) {
    case 64: launch_costate_l<KIND, NX, NU, 64, COMPACT, TP...>(p, w, mode, grid, s, tp...); break;
    case 32: launch_costate_l<KIND, NX, NU, 32, COMPACT, TP...>(p, w, mode, grid, s, tp...); break;
    case 16: launch_costate_l<KIND, NX, NU, 16, COMPACT, TP...>(p, w, mode, grid, s, tp...); break;
    case 8: launch_costate_l<KIND, NX, NU, 8, COMPACT, TP...>(p, w, mode, grid, s, tp...); break;
    default: launch_costate_l<KIND, NX, NU, 1, COMPACT, TP...>(p, w, mode, grid, s, tp...); break;
  }
}

template <int KIND, int NX, int NU, bool COMPACT, class... TP>
__global__ __launch_bounds__(256) void assemble_kernel(noc_family prm, noc_ipm_ws w, int terminal, TP... tp) {
  if constexpr (sizeof...(TP) > 0) {  // b = t / (chunk slots x lanes) per thread: vector loads
    const long long tt = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long per = (long long)((w.N + w.lanes - 1) / w.lanes) * w.lanes;
    if (tt >= (long long)w.Bt * per) return;  // keeps the record read in range
    load_traj_params<NX, NU>(prm, tp..., (int)(tt / per));
  }
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int N = w.N, L = w.lanes;
  const Chunks ch(N, L);
  if (t >= (long long)w.Bt * ch.cmax * L) return;
  const int b = (int)(t / ((long long)ch.cmax * L));
  const int rem = (int)(t % ((long long)ch.cmax * L));
  const int j = rem / L, l = rem % L;
  if (j >= ch.len(l) || !builds_blocks(w, b)) return;
  const int k = ch.start(l) + j;
  const size_t tn = (size_t)b * N + k;
  Fam<KIND, NX, NU> f(prm);
  const double bp = w.bp[b];
  double x[NX], u[NU], lam[NX];
  gload<NX>(w.x + ((size_t)b * (N + 1) + k) * NX, x);
  NOC_UNROLL for (int i = 0; i < NU; ++i) u[i] = w.u[tn * NU + i];
  gload<NX>(w.lam + ((size_t)b * (N + 1) + k + 1) * NX, lam);
  // Q = cxx + l.fxx ; R = cuu + l.fuu ; M = cxu + l.fxu  (P:35-37), l = lambda_{k+1}
  double Q[NX * NX], R[NU * NU], M[NX * NU];
  f.stage_hess(x, u, bp, Q, R, M);
  f.add_hess_l(x, u, lam, Q, R, M);
  Sym<NX> Qs;
  Sym<NU> Rs;
  NOC_UNROLL for (int i = 0; i < NX; ++i)
    NOC_UNROLL for (int jj = i; jj < NX; ++jj) Qs(i, jj) = (i == jj) ? Q[i * NX + i] : 0.5 * (Q[i * NX + jj] + Q[jj * NX + i]);
  NOC_UNROLL for (int i = 0; i < NU; ++i)
    NOC_UNROLL for (int jj = i; jj < NU; ++jj) Rs(i, jj) = (i == jj) ? R[i * NU + i] : 0.5 * (R[i * NU + jj] + R[jj * NU + i]);
  if constexpr (COMPACT) {
    using BS = BlockStruct<KIND, NX, NU, true>;
    constexpr int VQ = BS::template nv<BF_Q>(), VR = BS::template nv<BF_R>(), VM = BS::template nv<BF_M>();
    double vq[VQ > 0 ? VQ : 1], vr[VR > 0 ? VR : 1], vm[VM > 0 ? VM : 1];
    BS::template compress<BF_Q>(Qs.v, vq);
    BS::template compress<BF_R>(Rs.v, vr);
    BS::template compress<BF_M>(M, vm);
    if constexpr (VQ > 0) tstore_rt<VQ>(w.Q, L, ch.cmax, b, j, l, vq);
    if constexpr (VR > 0) tstore_rt<VR>(w.R, L, ch.cmax, b, j, l, vr);
    if constexpr (VM > 0) tstore_rt<VM>(w.M, L, ch.cmax, b, j, l, vm);
  } else {
    tstore_rt<Sym<NX>::SZ>(w.Q, L, ch.cmax, b, j, l, Qs.v);
    tstore_rt<Sym<NU>::SZ>(w.R, L, ch.cmax, b, j, l, Rs.v);
    tstore_rt<NX * NU>(w.M, L, ch.cmax, b, j, l, M);
  }
  if (terminal == NOC_TERMINAL_STAGE0 && k == 0) gstore<NX * NX>(w.P + (size_t)b * NX * NX, Q);  // P:73
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

template <int KIND, int NX, int NU, class... TP>
__global__ __launch_bounds__(256) void trial_kernel(noc_family prm, noc_ipm_ws w, int mode, TP... tp) {
  if constexpr (sizeof...(TP) > 0) {  // the trajectory is wave-uniform here: scalar loads
    const int bt = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (bt >= w.Bt) return;  // keeps the record read in range
    load_traj_params<NX, NU>(prm, tp..., __builtin_amdgcn_readfirstlane(bt));
  }
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (b >= w.Bt || w.phase[b] != NOC_PHASE_SOLVE) return;  // uniform per wave
  Fam<KIND, NX, NU> f(prm);
  const int N = w.N;
  const double bp = w.bp[b];
  const double* X = w.x + (size_t)b * (N + 1) * NX;
  const double* DX = w.dx + (size_t)b * (N + 1) * NX;
  const double* U = w.u + (size_t)b * N * NU;
  const double* DU = w.du + (size_t)b * N * NU;
  // lane l sums the stages of horizon chunk l (the 64-lane chunk geometry) and the last lane adds
  // the final cost: the same summation order as the persistent solver (ipm_persistent.hip), so
  // both drivers take identical accept / reject decisions
  double csum = 0.0;
  int ok = 1;
  const Chunks ch(N, 64);
  for (int k = ch.start(lane); k < ch.start(lane) + ch.len(lane); ++k) {
    double xt[NX], ut[NU];
    NOC_UNROLL for (int i = 0; i < NX; ++i) xt[i] = X[(size_t)k * NX + i] + DX[(size_t)k * NX + i];
    NOC_UNROLL for (int j = 0; j < NU; ++j) ut[j] = U[(size_t)k * NU + j] + DU[(size_t)k * NU + j];
    ok &= f.feasible(xt, ut) ? 1 : 0;
    csum += f.stage_cost(xt, ut, bp);
  }
  if (lane == 63) {
    double xt[NX];
    NOC_UNROLL for (int i = 0; i < NX; ++i) xt[i] = X[(size_t)N * NX + i] + DX[(size_t)N * NX + i];
    csum += f.final_cost(xt);
  }
  csum = wave_sum(csum);
  const bool traj_ok = __all(ok);
  // new_cost = where(feasible, total_cost(trial), inf)   (P:159-163, S:126-129)
  const double new_cost = traj_ok ? csum : INFINITY;
  // the accept rule and barrier schedule of every solver (ipm_schedule.h); no solve cap here, so
  // the retry accounting has the whole retry loop for room
  IpmState s;
  s.load(w, b);
  const AcceptOutcome o = accept_step(s, mode, new_cost, w.pred[b], w.feasible[b] != 0, w.flags, 501);
  if (o.take) {  // x <- x + dx, u <- u + du
    double* Xw = w.x + (size_t)b * (N + 1) * NX;
    double* Uw = w.u + (size_t)b * N * NU;
    for (int k = lane; k <= N; k += 64) {
      NOC_UNROLL for (int i = 0; i < NX; ++i) Xw[(size_t)k * NX + i] += DX[(size_t)k * NX + i];
      if (k < N) NOC_UNROLL for (int j = 0; j < NU; ++j) Uw[(size_t)k * NU + j] += DU[(size_t)k * NU + j];
    }
  }
  if (lane != 0) return;
  if (w.repeats) w.repeats[b] += o.rep;
  w.kkt_solves[b] = s.solves;
  w.inner[b] = s.inner;
  w.it[b] = s.it;
  w.rp[b] = s.rp;
  w.rinc[b] = s.rinc;
  if (o.stage_done) {
    w.total_it[b] = s.total_it;
    w.bp[b] = s.bp;
  }
  // the rollout of a new stage happens in the next step (ROLLOUT_PENDING, see rollout_kernel)
  int phase = resume_point(o.stage_done, o.relinearize, s.bp, w.flags);
  if (phase == NOC_PHASE_ROLLOUT) phase = NOC_PHASE_ROLLOUT_PENDING;
  if (phase == NOC_PHASE_SOLVE) w.reg[b] = candidate_reg(mode, s.rp, s.gnorm);
  w.phase[b] = phase;
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
template <int KIND, int NX, int NU, bool COMPACT, class... TP>
static hipError_t prepare_main_c(const noc_family& p, const noc_ipm_ws& w, int mode, int terminal,
                                 hipStream_t s, TP... tp) {
  const int bt_grid = (w.Bt + 255) / 256;
  const long long cmax = (w.N + w.lanes - 1) / w.lanes;
  const unsigned st_grid = (unsigned)(((long long)w.Bt * cmax * w.lanes + 255) / 256);
  hipLaunchKernelGGL((linearize_kernel<KIND, NX, NU, COMPACT, TP...>), dim3(st_grid), dim3(256), 0, s, p, w, tp...);
  launch_costate<KIND, NX, NU, COMPACT, TP...>(p, w, mode, s, tp...);  // TP named: deduction would drop its restrict
  hipLaunchKernelGGL((assemble_kernel<KIND, NX, NU, COMPACT, TP...>), dim3(st_grid), dim3(256), 0, s, p, w, terminal, tp...);
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

hipError_t ipm_promote(const noc_ipm_ws& w, hipStream_t s) {
  hipLaunchKernelGGL(promote_kernel, dim3((w.Bt + 255) / 256), dim3(256), 0, s, w);
  return hipGetLastError();
}

// family dispatch (ipm_family.h: for_family): one instantiation per NOC_FAMILY line of families.def
// Rollout (it takes no tp: it reads dt and the dynamics only), promote, then the main part.  The
// families' dense and compact instances come first and the ones that take tp after them, in two
// passes, so the unit's kernels keep their order.
hipError_t ipm_prepare(const noc_family& p, const noc_ipm_ws& w, int mode, int terminal,
                       bool compact, const double* tp, hipStream_t s) {
  if (tp && compact) return hipErrorInvalidValue;
  const auto roll = [&](auto K, auto X, auto U) {
    const hipError_t e = rollout_t<K, X, U>(p, w, s, 1);
    if (e == hipSuccess) hipLaunchKernelGGL(promote_kernel, dim3((w.Bt + 255) / 256), dim3(256), 0, s, w);
    return e;
  };
  if (!tp)
    return for_family(p, hipErrorInvalidValue, [&](auto K, auto X, auto U) {
      const hipError_t e = roll(K, X, U);
      return e != hipSuccess ? e : prepare_main_t<K, X, U>(p, w, mode, terminal, compact, s);
    });
  return for_family(p, hipErrorInvalidValue, [&](auto K, auto X, auto U) {
    if constexpr (traj_params_instance<K, X, U>()) {
      const hipError_t e = roll(K, X, U);
      return e != hipSuccess ? e : prepare_main_c<K, X, U, false, TrajParams>(p, w, mode, terminal, s, tp);
    } else {
      return hipErrorInvalidValue;
    }
  });
}

hipError_t ipm_rollout(const noc_family& p, const noc_ipm_ws& w, hipStream_t s) {
  return for_family(p, hipErrorInvalidValue, [&](auto K, auto X, auto U) { return rollout_t<K, X, U>(p, w, s, 0); });
}

hipError_t ipm_prepare_main(const noc_family& p, const noc_ipm_ws& w, int mode, int terminal,
                            bool compact, hipStream_t s) {
  return for_family(p, hipErrorInvalidValue, [&](auto K, auto X, auto U) {
    return prepare_main_t<K, X, U>(p, w, mode, terminal, compact, s);
  });
}

// tp: nothing, or the records (a TrajParams)
template <class... TP>
static hipError_t launch_trial(const noc_family& p, const noc_ipm_ws& w, int mode, hipStream_t s, TP... tp) {
  return for_family(p, hipErrorInvalidValue, [&](auto K, auto X, auto U) {
    if constexpr (sizeof...(TP) > 0 && !traj_params_instance<K, X, U>()) {
      return hipErrorInvalidValue;
    } else {
      hipLaunchKernelGGL((trial_kernel<K, X, U, TP...>), dim3((unsigned)((w.Bt + 3) / 4)), dim3(256), 0, s, p, w,
                         mode, tp...);
      return hipGetLastError();
    }
  });
}

hipError_t ipm_trial(const noc_family& p, const noc_ipm_ws& w, int mode, const double* tp,
                     hipStream_t s) {
  return !tp ? launch_trial(p, w, mode, s) : launch_trial<TrajParams>(p, w, mode, s, tp);
}

hipError_t ipm_init(const noc_ipm_ws& w, double bp0, hipStream_t s) {
  hipLaunchKernelGGL(init_kernel, dim3((w.Bt + 255) / 256), dim3(256), 0, s, w, bp0);
  return hipGetLastError();
}

// the library has instances for p (a families.def line) ...
bool family_supported(const noc_family& p) {
  return for_family(p, false, [](auto, auto, auto) { return true; });
}

// ... with the parametrised quadratic cost (not a registered family's traced costs)
bool traj_params_supported(const noc_family& p) {
  return for_family(p, false, [](auto K, auto X, auto U) { return traj_params_instance<K, X, U>(); });
}

}  // namespace noc
