// Interior-point DDP on the MI355X: the reference's third solver
// (noc/differential_dynamic_programming.py, "D"), the whole barrier schedule of every trajectory
// in ONE launch, one wave64 per trajectory.
//
// DDP's backward pass is NOT the KKT scan: its Q-function carries the second-order dynamics terms
// Vx . fxx evaluated with the pass's own value gradient Vx_{k+1} (D:43-45), so the recursion is
// nonlinear in V and has no associative form; the forward pass is the nonlinear closed-loop
// rollout (D:73-90).  Both recursions are horizon-sequential.  What is NOT sequential is the
// expensive part of a backward step -- the stage derivatives at the nominal (x, u) (the generated
// family code: sincos, divisions), which are the same for every retry of an iteration.  So:
//   * derivatives: the 64 lanes evaluate them stage-parallel once per DDP iteration into a
//     per-stage record (fx, fu, cx, cu, cuu and the full second-derivative tensors d2f_i, taken
//     as add_hess_l with l = e_i), written to HBM / L2;
//   * backward pass: wave-uniform (every lane runs the same recursion; lane 0 stores k, K),
//     reading the records -- only the Vx contraction and the Riccati-like algebra remain;
//   * rollouts: wave-uniform recurrence (lane 0 stores), then trial cost and feasibility
//     stage-parallel with wave reductions (cost summed chunk-wise in stage order, then across
//     lanes: the summation order of the multi-lane Newton kernels).
// Every wave follows its own trajectory's reference control flow (outer Newton loop D:105-170,
// retry loop D:114-152, barrier loop D:189-208; the clip, the retry cap, the retry accounting and
// the barrier step are the interior-point solvers': ipm_schedule.h).  Layout: natural, per
// trajectory contiguous (x (Bt, N+1, nx), u (Bt, N, nu)); workspace include/noc_hip.h
// noc_ddp_work_doubles.
#include <hip/hip_runtime.h>
#include <cstdlib>

#include <cmath>

#include "../../include/noc_hip.h"
#include "ipm_family.h"
#include "ipm_schedule.h"
#include "noc_internal.h"

namespace noc {

// Diagnostic per-pass trace of the DDP decisions (tools/ddp_trace_diff.py), set by the debug
// export noc_debug_set_ddp_trace (not part of the ABI header); NULL in product use.
__device__ double* g_ddp_trace = nullptr;
__device__ int g_ddp_trace_cap = 0;
__device__ int g_ddp_trace_traj = 0;

struct DdpArgs {
  int N, Bt, max_passes;
  int skip_repeats;  // account the identical retries at the rp clip without recomputing them
  int one_stage;     // NOC_DDP_ONE_STAGE: ddp(ocp, u, x0, bp) -- one barrier value (D:98-186)
  double bp0;
  const double* x0;
  double* u;
  double *X, *TX, *TU, *k, *K, *rec;
  int *iterations, *passes, *done;
};

// per-stage derivative record: fx | fu | cx | cu | cxx | cuu | cxu (the stage cost's full Hessian,
// D:43-45 -- a registered family's traced cost is not diagonal) | Hxx_i | Hxu_i | Huu_i (i < nx)
template <int NX, int NU>
struct Rec {
  static constexpr int FX = 0, FU = FX + NX * NX, CX = FU + NX * NU, CU = CX + NX, CXX = CU + NU,
                       CUU = CXX + NX * NX, CXU = CUU + NU * NU, HXX = CXU + NX * NU,
                       HXU = HXX + NX * NX * NX, HUU = HXU + NX * NX * NU,
                       SIZE = HUU + NX * NU * NU;
};

NOC_DEV void ddp_fence() { __threadfence_block(); }  // this wave's global stores before its loads

template <int KIND, int NX, int NU>
__global__ __launch_bounds__(64) void ddp_solve_kernel(noc_family prm, DdpArgs a) {
#include "ddp_solve_body.h"
}

// Per-trajectory cost parameters (noc_ddp_solve_params): the same body on a family argument that
// first takes goal, wx, wu, wf, u_bound of the workgroup's trajectory from its record in tp
// (Bt, NOC_TRAJ_PARAM_DOUBLES).  One wave per trajectory and no order permutation: the record
// index is the workgroup index, wave-uniform by construction, and the loads come before any
// store, so the record arrives as scalar loads and the fields stay scalar operands like kernel
// arguments.  Every consumer of a cost parameter in the body reads `prm` (Fam, and prm.wx for the
// backward pass's Qxx diagonal), so all of them see the trajectory's values.
template <int KIND, int NX, int NU>
__global__ __launch_bounds__(64) void ddp_solve_params_kernel(noc_family prm, DdpArgs a,
                                                              const double* __restrict__ tp) {
  {
    const int bt = blockIdx.x;
    if (bt >= a.Bt) return;  // as the body: keeps the record read in range
    load_traj_params<NX, NU>(prm, tp, bt);
  }
#include "ddp_solve_body.h"
}

// instances for nx <= 4 only (a template: the others are never instantiated); tp != NULL: the
// params kernel, for the families with the parametrised cost only
template <int K, int X, int U>
static hipError_t ddp_family(const noc_family& p, const DdpArgs& a, const double* tp, hipStream_t s) {
  if constexpr (X <= 4) {
    if (!tp) {
      hipLaunchKernelGGL((ddp_solve_kernel<K, X, U>), dim3(a.Bt), dim3(64), 0, s, p, a);
      return hipGetLastError();
    }
    if constexpr (!Fam<K, X, U>::kGenCost) {
      hipLaunchKernelGGL((ddp_solve_params_kernel<K, X, U>), dim3(a.Bt), dim3(64), 0, s, p, a, tp);
      return hipGetLastError();
    }
  }
  return hipErrorInvalidValue;
}

bool ddp_supported(const noc_family& p) {
  // any registered family's cost (parametrised or traced: the record holds the full Hessian);
  // nx <= 4: every lane holds the value Hessian and the stage's Q blocks in registers
  return family_supported(p) && p.nx <= 4;
}

long long ddp_record_doubles(int nx, int nu) {
  return (long long)nx * nx + nx * nu + nx + nu + (long long)nx * nx + nu * nu + nx * nu +
         (long long)nx * (nx * nx + nx * nu + nu * nu);
}

bool ddp_params_supported(const noc_family& p) {
  return ddp_supported(p) && traj_params_supported(p);  // the parametrised cost, nx <= 4
}

// tp: NULL, or the (Bt, 32) per-trajectory parameter records (ddp_params_supported families)
static hipError_t ddp_launch(const noc_family& p, int N, int Bt, const double* x0, double* u,
                             double* work, int* iterations, int* passes, int* done, double bp0,
                             int max_passes, int flags, const double* tp, hipStream_t s) {
  DdpArgs a{};
  a.one_stage = (flags & NOC_DDP_ONE_STAGE) ? 1 : 0;
  a.N = N;
  a.Bt = Bt;
  a.max_passes = max_passes;
  const char* no_skip = std::getenv("NOC_DDP_NO_REPEAT_SKIP");  // 1: recompute every retry
  a.skip_repeats = !(no_skip && no_skip[0] == '1');
  a.bp0 = bp0;
  a.x0 = x0;
  a.u = u;
  const size_t nxs = (size_t)Bt * (N + 1) * p.nx, nus = (size_t)Bt * N * p.nu;
  a.X = work;
  a.TX = a.X + nxs;
  a.TU = a.TX + nxs;
  a.k = a.TU + nus;
  a.K = a.k + nus;
  a.rec = a.K + nus * p.nx;
  a.iterations = iterations;
  a.passes = passes;
  a.done = done;
#define NOC_FAMILY(K, X, U) \
  if (p.kind == K && p.nx == X && p.nu == U) return ddp_family<K, X, U>(p, a, tp, s);
#include NOC_FAMILIES_DEF
#undef NOC_FAMILY
  return hipErrorInvalidValue;
}

hipError_t ddp_solve(const noc_family& p, int N, int Bt, const double* x0, double* u,
                     double* work, int* iterations, int* passes, int* done, double bp0,
                     int max_passes, int flags, hipStream_t s) {
  return ddp_launch(p, N, Bt, x0, u, work, iterations, passes, done, bp0, max_passes, flags,
                    nullptr, s);
}

hipError_t ddp_solve_params(const noc_family& p, int N, int Bt, const double* x0, double* u,
                            double* work, int* iterations, int* passes, int* done,
                            const double* tp, double bp0, int max_passes, int flags,
                            hipStream_t s) {
  if (!tp || !ddp_params_supported(p)) return hipErrorInvalidValue;
  return ddp_launch(p, N, Bt, x0, u, work, iterations, passes, done, bp0, max_passes, flags, tp, s);
}

}  // namespace noc

// debug export: trace buffer of traj x cap x 10 doubles (bp, it, inner, pred, gain, success, rp,
// |Hu|, cost, new_cost per backward pass) for the first `traj` trajectories; buf = NULL disables
extern "C" int noc_debug_set_ddp_trace(double* buf, int cap, int traj) {
  if (hipMemcpyToSymbol(HIP_SYMBOL(noc::g_ddp_trace), &buf, sizeof(buf)) != hipSuccess) return -1;
  if (hipMemcpyToSymbol(HIP_SYMBOL(noc::g_ddp_trace_cap), &cap, sizeof(cap)) != hipSuccess) return -1;
  if (hipMemcpyToSymbol(HIP_SYMBOL(noc::g_ddp_trace_traj), &traj, sizeof(traj)) != hipSuccess) return -1;
  return 0;
}
