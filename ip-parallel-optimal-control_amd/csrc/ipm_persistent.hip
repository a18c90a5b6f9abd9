// Persistent batched interior-point solver: the WHOLE barrier schedule of one trajectory in one
// wave64, one launch for the batch (fp64, gfx950).
//
// Replaces par_interior_point_optimal_control / newton_oc (noc/par_interior_point_newton.py:
// 127-254) and, with NOC_MODE_SEQ, seq_interior_point_optimal_control (noc/seq_interior_point_
// newton.py:108-202), for registered families.  Every trajectory runs its own reference control
// flow back to back -- rollout, linearise, costates, LQ blocks, KKT scan, trial / accept /
// regularisation, Newton stop test, barrier schedule -- with no kernel boundary, no host poll and
// no all-trajectory lockstep: a trajectory that needs 850 Newton steps no longer holds 4095 others
// in per-step launches, and the per-step launch overhead is gone.
//
// The accept rule and barrier schedule are every solver's (ipm_schedule.h) and the arithmetic is
// the multi-launch driver's (ipm_kernels.hip + the KKT scan kernel at lanes = 64), so both
// produce identical iterates.  Lane l owns the horizon chunk of
// the tiled layout (workspace lanes must be 64); cross-lane data moves through shuffles, the
// KKT step stays in LDS (kkt_scan_wave with lds_out and dx = du = NULL), and the few hand-offs
// through the workspace (rollout states, pred / feasible, the terminal Hessian) are ordered by a
// workgroup fence (one wave = one workgroup).
#include <hip/hip_runtime.h>
#include <cstdlib>

#include "../../include/noc_hip.h"
#include "block_struct.h"
#include "ipm_family.h"
#include "ipm_plan.h"
#include "ipm_schedule.h"
#include "kkt_compact_src.h"
#include "kkt_scan_impl.h"
#include "noc_internal.h"

namespace noc {

// Per-phase cycle counters of workgroup 0 (timing-only instrumentation; built only with
// -DNOC_PERSIST_PROFILE, read back by noc_debug_phase_cycles): rollout, linearise, costate +
// blocks, KKT scan, trial, number of Newton iterations.
__device__ long long g_phase_cycles[8];  // [6]: the trial's costs + reductions; [7]: the costate scan
// Start / end wall-clock stamps (s_memrealtime, 100 MHz) of every trajectory's persistent solve,
// same builds only (read back by noc_debug_traj_times): the batch's schedule, e.g. when the
// straggler that sets the wall time started and how its neighbours thinned out.
constexpr int kTrajStamps = 16384;
__device__ long long g_traj_times[kTrajStamps][2];
// decision trace (-DNOC_DECISION_TRACE builds only; noc_internal.h)
__device__ DecisionTrace g_dtrace;

namespace {
constexpr int PL = 64;  // lanes per trajectory in the persistent solver

NOC_DEV void wave_fence() { __threadfence_block(); }

// The solver state (IpmState, ipm_schedule.h) is parked in LDS across the KKT scan (whose register
// footprint is the kernel's peak) instead of being kept live in VGPRs through it.
// Speculative candidates (SPEC > 1 waves per trajectory, one candidate regularisation each): the
// scan's reg / pred / feasible of a wave's candidate, and its trial cost, exchanged through LDS.
struct SpecIO {
  double reg, pred, new_cost, pad;
  int feasible, pad2[3];
};

// LDS of one workgroup: the layout and its sizes are ipm_plan.h's (the launch is sized by the same
// functions); here with the kernels' template constants.
static_assert(sizeof(IpmState) == kIpmStateBytes && sizeof(SpecIO) == kSpecIOBytes, "ipm_plan.h sizes the LDS");
template <int NX, int NU>
__host__ __device__ constexpr int slot_doubles(int N) { return noc::slot_doubles(NX, NU, N); }
template <int NX, int NU>
NOC_DEV IpmState* state_slot(int N, int spec = 1, int wv = 0) {
  extern __shared__ __attribute__((aligned(16))) double noc_smem[];
  return reinterpret_cast<IpmState*>(noc_smem + spec * slot_doubles<NX, NU>(N) + wv * state_doubles());
}
template <int NX, int NU>
NOC_DEV SpecIO* spec_io(int N, int spec, int wv) {
  extern __shared__ __attribute__((aligned(16))) double noc_smem[];
  return reinterpret_cast<SpecIO*>(noc_smem + spec * (slot_doubles<NX, NU>(N) + state_doubles())) + wv;
}

// XLDS instances: the trajectory's states and controls x[0..N], u[0..N-1] live in LDS for the
// whole solve (the rollout, linearisation, costate sweep, trial and update all read or write
// them; from the workspace each access was a global round trip), copied in at the start and out
// at the end.  Layout behind the KKT slots and the parked state: x [(N+1) NX], u [N NU].
template <int NX, int NU>
__host__ __device__ constexpr int xlds_off(int N, int spec = 1, int wv = 0) { return noc::xlds_off(NX, NU, N, spec, wv); }

}  // namespace

#ifdef NOC_PERSIST_PROFILE
#define NOC_PHASE(i) do { const long long t_ = clock64(); if (b == 0 && lead) g_phase_cycles[i] += t_ - t_prev; t_prev = t_; } while (0)
// a sub-phase ending now, started at t0 (does not move t_prev)
#define NOC_SUB(i, t0) do { if (b == 0 && lead) g_phase_cycles[i] += clock64() - (t0); } while (0)
#define NOC_T0(v) const long long v = clock64()
#else
#define NOC_PHASE(i) do { } while (0)
#define NOC_SUB(i, t0) do { } while (0)
#define NOC_T0(v) do { } while (0)
#endif

// WPS: waves per SIMD the register budget is sized for.  2 = 256 registers per lane; 1 = 512, the
// upper half AGPRs, which the compiler uses as spill space instead of scratch (cart-pole: 460 B
// of scratch per lane at WPS = 2, none at WPS = 1), and which pays for the stage pairs below.
// RESUME: continue from the workspace state (NOC_WS_RESUME; its own instance, so the plain solve's
// register allocation does not carry the resume bookkeeping).
// STRUCT: the structure-aware blocks (block_struct.h; NOC_PERSIST_STRUCT=0 selects the dense
// instance, which computes the same doubles).
// SPEC: waves per trajectory, each solving one candidate of the regularisation's failure chain
// (speculative retries, below); 1 = the plain solver.  SPEC > 1 needs XLDS (every wave keeps its
// own copy of x, u).
// This kernel keeps a twin for the per-trajectory records, ipm_solve_params_kernel, and the two
// share their body through ipm_solve_body.h, included between their braces: folded into one
// kernel like the building blocks, by a trailing argument pack or by a force-inlined body
// function, cart-pole instances' scratch moved (profiles/r10/params_fold/README.md).  The twin
// (noc_ipm_solve_params) is the one-wave solver on structure-aware blocks (STRUCT, SPEC = 1): the
// family argument first takes goal, wx, wu, wf, u_bound of the workgroup's trajectory from its record in
// tp (Bt, NOC_TRAJ_PARAM_DOUBLES).  The record follows the trajectory, not the workgroup (w.order
// permutes workgroups); the index is wave-uniform (said to the compiler by readfirstlane) and the
// loads come before any store, so the record arrives as one scalar burst and the fields stay
// scalar operands like kernel arguments.  Every consumer -- Fam, the BK_WX constants of
// fold_consts / expand and of the inlined KKT scan's CompactSrc -- reads `prm`, so none is missed.
template <int KIND, int NX, int NU, int WPS, bool RESUME, bool XLDS, bool STRUCT, int SPEC = 1>
__global__ __launch_bounds__(64 * SPEC, WPS) void ipm_solve_kernel(noc_family prm, noc_ipm_ws w, int mode,
                                                                int terminal, double bp0,
                                                                int max_solves) {
#include "ipm_solve_body.h"
}

template <int KIND, int NX, int NU, int WPS, bool RESUME, bool XLDS>
__global__ __launch_bounds__(64, WPS) void ipm_solve_params_kernel(noc_family prm, noc_ipm_ws w,
                                                                   const double* __restrict__ tp, int mode,
                                                                   int terminal, double bp0, int max_solves) {
  constexpr bool STRUCT = true;
  constexpr int SPEC = 1;
  {
    const int bt = w.order ? w.order[blockIdx.x] : (int)blockIdx.x;
    if (bt < 0 || bt >= w.Bt) return;  // as the body: an out-of-range order entry solves nothing
    load_traj_params<NX, NU>(prm, tp, __builtin_amdgcn_readfirstlane(bt));
  }
#include "ipm_solve_body.h"
}

// Constant dispatch, as for_family: fn(std::integral_constant<int, V>) for the V of Vs... equal to
// v -- a run-time value of the plan as a template argument of the instance -- and its result;
// `none` if v is none of them.
template <int... Vs, class R, class Fn>
inline R for_const(int v, R none, Fn&& fn) {
  R r = none;
  (void)((v == Vs && ((void)(r = fn(std::integral_constant<int, Vs>{})), true)) || ...);
  return r;
}

struct SolveArgs {
  const noc_family& p;
  const double* tp;  // per-trajectory records (noc_ipm_solve_params) or NULL
  int mode, terminal;
  double bp0;
  int max_solves;
};

// One launch of the plan: the instance its fields name.  The instances that exist: SPEC > 1 only
// at WPS = 1 with XLDS and STRUCT, the per-trajectory twin only at STRUCT and SPEC = 1, WPS = 1
// only for the families with a one-wave instance.  (The value lists are in the order that keeps
// the unit's kernels where they were in its device code.)
template <int KIND, int NX, int NU>
static hipError_t launch_one(const PersistLaunch& L, const SolveArgs& a, const noc_ipm_ws& w, hipStream_t s) {
  const hipError_t none = hipErrorInvalidValue;
  const dim3 grid(L.grid), block(64 * L.spec);
  const size_t lds = (size_t)L.lds;
  return for_const<1, 4, 2>(L.spec, none, [&](auto SPEC) {
    return for_const<2, 1>(L.wps, none, [&](auto WPS) {
      return for_const<0, 1>(L.xlds, none, [&](auto XLDS) {
        return for_const<0, 1>(L.resume, none, [&](auto RES) {
          if constexpr ((WPS == 1 && !one_wave_instance(KIND)) || (SPEC > 1 && !(WPS == 1 && XLDS))) {
            return none;
          } else if constexpr (SPEC > 1) {
            if (a.tp || !L.strct) return none;
            hipLaunchKernelGGL((ipm_solve_kernel<KIND, NX, NU, WPS, RES, XLDS, true, SPEC>), grid, block, lds, s,
                               a.p, w, a.mode, a.terminal, a.bp0, a.max_solves);
            return hipGetLastError();
          } else {
            if (a.tp)
              hipLaunchKernelGGL((ipm_solve_params_kernel<KIND, NX, NU, WPS, RES, XLDS>), grid, block, lds, s,
                                 a.p, w, a.tp, a.mode, a.terminal, a.bp0, a.max_solves);
            else if (!L.strct)
              hipLaunchKernelGGL((ipm_solve_kernel<KIND, NX, NU, WPS, RES, XLDS, false>), grid, block, lds, s,
                                 a.p, w, a.mode, a.terminal, a.bp0, a.max_solves);
            else
              hipLaunchKernelGGL((ipm_solve_kernel<KIND, NX, NU, WPS, RES, XLDS, true>), grid, block, lds, s,
                                 a.p, w, a.mode, a.terminal, a.bp0, a.max_solves);
            return hipGetLastError();
          }
        });
      });
    });
  });
}

// The heavy-first split (ipm_plan.h: plan_heavy): plan.main on the first plan.heavy entries of
// w.order, concurrently with plan.rest on the others (second stream, event fork / join).
template <int KIND, int NX, int NU>
static hipError_t launch_split(const PersistPlan& plan, const SolveArgs& a, const noc_ipm_ws& w, hipStream_t s) {
  thread_local hipStream_t s2 = nullptr;
  thread_local hipEvent_t fork = nullptr, join = nullptr;
  if (!s2) {
    if (hipStreamCreateWithFlags(&s2, hipStreamNonBlocking) != hipSuccess) return hipErrorUnknown;
    if (hipEventCreateWithFlags(&fork, hipEventDisableTiming) != hipSuccess) return hipErrorUnknown;
    if (hipEventCreateWithFlags(&join, hipEventDisableTiming) != hipSuccess) return hipErrorUnknown;
  }
  hipError_t e;
  if ((e = hipEventRecord(fork, s)) != hipSuccess) return e;
  if ((e = hipStreamWaitEvent(s2, fork, 0)) != hipSuccess) return e;
  // the heavy launch first, so its workgroups are placed before the two-wave ones fill the SIMDs
  if ((e = launch_one<KIND, NX, NU>(plan.main, a, w, s)) != hipSuccess) return e;
  noc_ipm_ws rest = w;
  rest.order = w.order + plan.heavy;
  if ((e = launch_one<KIND, NX, NU>(plan.rest, a, rest, s2)) != hipSuccess) return e;
  if ((e = hipEventRecord(join, s2)) != hipSuccess) return e;
  return hipStreamWaitEvent(s, join, 0);
}

int debug_phase_cycles(long long* out, int n, int reset) {
  long long host[8], sub[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (hipMemcpyFromSymbol(host, HIP_SYMBOL(g_phase_cycles), sizeof(host)) != hipSuccess) return -1;
#ifdef NOC_PERSIST_PROFILE  // the one-wave kernel's KKT sub-phases (kkt_scan_impl.h: NOC_STAMP)
  if (hipMemcpyFromSymbol(sub, HIP_SYMBOL(g_scan_sub), sizeof(sub)) != hipSuccess) return -1;
#endif
  long long wide[16];
  if (debug_wide_cycles(wide, 16, reset) != 0) return -1;  // the wide kernel's (ipm_wide.hip)
  for (int i = 0; i < n && i < 16; ++i) out[i] = (i < 8 ? host[i] : sub[i - 8]) + wide[i];
  if (reset) {
    const long long zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_phase_cycles), zero, sizeof(zero)) != hipSuccess) return -1;
#ifdef NOC_PERSIST_PROFILE
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_scan_sub), zero, sizeof(zero)) != hipSuccess) return -1;
#endif
  }
  return 0;
}

// decision-trace buffer of both persistent kernels; 1 if this build records (NOC_DECISION_TRACE),
// 0 if it has no trace code, -1 on a HIP error
int debug_set_decision_trace(double* buf, int cap, int ntraj) {
  const DecisionTrace t{buf, cap, ntraj};
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_dtrace), &t, sizeof(t)) != hipSuccess) return -1;
  if (wide_set_decision_trace(t) != 0) return -1;
#ifdef NOC_DECISION_TRACE
  return 1;
#else
  return 0;
#endif
}

int debug_traj_times(long long* out, int n) {
  if (n > kTrajStamps) n = kTrajStamps;
  if (n <= 0) return 0;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_traj_times), (size_t)n * 2 * sizeof(long long)) ==
                 hipSuccess ? 0 : -1;
}

bool ipm_solve_supported(const noc_family& p, int N, int lanes) {
  return lanes == PL && family_supported(p) && persistent_instance(p.nx) && onewave_lds_bytes(p.nx, p.nu, N) > 0;
}

// The plan of one solve call (ipm_plan.h) for the environment as it is now.  simds = 0: the
// current device's (then 0 if none is visible); with_params: a solve with tp.
static PersistPlan ipm_plan(const noc_family& p, int N, int Bt, bool ordered, int flags, bool with_params,
                            int simds) {
  if (!family_supported(p) || (with_params && !traj_params_supported(p))) return PersistPlan{};
  PersistQuery q{p.kind, p.nx, p.nu, N, Bt, ordered, flags, with_params, simds ? simds : device_simds(0), 0, 0};
  if (!with_params && ipm_wide_supported(p, N)) {
    q.wide_lds2 = (long long)wide_lds_bytes(p, N, 2);
    q.wide_lds4 = (long long)wide_lds_bytes(p, N, 4);
  }
  return plan_persist(q, read_persist_knobs());
}

// noc_debug_ipm_plan: the plan's fields at out[NOC_PLAN_*] (include/noc_hip.h)
void debug_ipm_plan(const noc_family& p, int N, int Bt, int flags, bool ordered, bool with_params, int simds,
                    int* out) {
  const PersistPlan plan = ipm_plan(p, N, Bt, ordered, flags, with_params, simds);
  for (int i = 0; i < NOC_PLAN_INTS; ++i) out[i] = 0;
  out[NOC_PLAN_FAMILY] = plan.family;
  out[NOC_PLAN_WIDE_WAVES] = plan.wide_waves;
  out[NOC_PLAN_WIDE_LDS] = (int)plan.wide_lds;
  if (plan.family != PersistPlan::kOneWave) return;
  out[NOC_PLAN_HEAVY] = plan.heavy;
  const PersistLaunch* ls[2] = {&plan.main, &plan.rest};
  for (int i = 0; i < (plan.heavy > 0 ? 2 : 1); ++i) {
    int* o = out + (i ? NOC_PLAN_REST : NOC_PLAN_MAIN);
    const PersistLaunch& l = *ls[i];
    o[NOC_PLAN_WPS] = l.wps; o[NOC_PLAN_SPEC] = l.spec; o[NOC_PLAN_RESUME] = l.resume; o[NOC_PLAN_XLDS] = l.xlds;
    o[NOC_PLAN_STRUCT] = l.strct; o[NOC_PLAN_GRID] = l.grid; o[NOC_PLAN_LDS] = (int)l.lds;
  }
}

static hipError_t launch_plan(const PersistPlan& plan, const noc_ipm_ws& w, const SolveArgs& a, hipStream_t s) {
  if (plan.family == PersistPlan::kWide)
    return ipm_solve_wide(a.p, w, a.mode, a.terminal, a.bp0, a.max_solves, nullptr, nullptr, w.Bt,
                          plan.wide_waves, s);
  if (plan.family != PersistPlan::kOneWave) return hipErrorInvalidValue;  // use the launch driver
  return for_family(a.p, hipErrorInvalidValue, [&](auto K, auto X, auto U) {
    if constexpr (persistent_instance(X))
      return plan.heavy > 0 ? launch_split<K, X, U>(plan, a, w, s) : launch_one<K, X, U>(plan.main, a, w, s);
    else
      return hipErrorInvalidValue;
  });
}

// tp (per-trajectory cost parameters, noc_ipm_solve_params): the plan never gives them the wide
// kernel, speculative candidates or the heavy-first split (ipm_plan.h).
hipError_t ipm_solve(const noc_family& p, const noc_ipm_ws& w, int mode, int terminal, double bp0,
                     int max_solves, const double* tp, hipStream_t s) {
  const PersistPlan plan = ipm_plan(p, w.N, w.Bt, w.order != nullptr, w.flags, tp != nullptr, 0);
  return launch_plan(plan, w, SolveArgs{p, tp, mode, terminal, bp0, max_solves}, s);
}

}  // namespace noc
