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

// LDS of one workgroup, in doubles: SPEC regions of KKT slots (lds_slots: one per 64-lane
// segment), SPEC parked states, SPEC SpecIO records (SPEC > 1 only), then SPEC copies of x, u
// (XLDS).  SPEC = 1 is the one-wave layout: [slots][state][x, u].
template <int NX, int NU>
__host__ __device__ constexpr int slot_doubles(int N) { return (N * kd_width<NX, NU>() + NX + 1) & ~1; }
__host__ __device__ constexpr int state_doubles() { return (int)((sizeof(IpmState) + 15) / 16) * 2; }
__host__ __device__ constexpr int specio_doubles(int spec) { return spec > 1 ? (int)(sizeof(SpecIO) / 8) * spec : 0; }
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
__host__ __device__ constexpr int xlds_doubles(int N) { return ((N + 1) * NX + N * NU + 1) & ~1; }
template <int NX, int NU>
__host__ __device__ constexpr int xlds_off(int N, int spec = 1, int wv = 0) {
  return spec * (slot_doubles<NX, NU>(N) + state_doubles()) + specio_doubles(spec) + wv * xlds_doubles<NX, NU>(N);
}

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

// LDS of one persistent workgroup: the trajectory's KKT slots + the parked state.  Up to 64 KB
// (long horizons at small batch, e.g. the reference's N = 1000 timing runs: 2 workgroups per CU).
static size_t solve_lds_bytes(int nx, int nu, int N) {
  const size_t slots = (size_t)(((long long)N * nu * (nx + 1) + nx + 1) & ~1LL) * sizeof(double);
  const size_t bytes = slots + sizeof(IpmState) + 16;
  return bytes <= 65536 ? bytes : 0;
}

// SIMDs of the current device (4 per CU); 0 if the query fails
static int device_simds() {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
  return 4 * cus;
}

// Families whose kernel spills at 2 waves per SIMD (cart-pole) get a second instance at 1 wave per
// SIMD (512 registers per lane: no scratch, stage pairs), used when the batch fits one wave per
// SIMD anyway (B <= 4 x CUs: the reference's B = 1 runs, c2-sized batches); larger batches keep 2
// waves per SIMD for latency hiding.  The others stay at 2 waves (their 1-wave instance measured
// 5-7 % slower at B = 1).  NOC_PERSIST_WAVES=1|2 overrides the choice (timing experiments).
template <int KIND>
constexpr bool one_wave_instance() { return KIND == NOC_FAMILY_CARTPOLE; }

// grid: workgroups = the entries of w.order this launch solves (w.Bt without an order)
template <int KIND, int NX, int NU, int WPS, bool RESUME, bool XLDS>
static hipError_t launch_solve(const noc_family& p, const noc_ipm_ws& w, int mode, int terminal,
                               double bp0, int max_solves, size_t lds, hipStream_t s, int grid,
                               const double* tp = nullptr) {
  if (tp) {  // per-trajectory parameters: the structure-aware instance only
    hipLaunchKernelGGL((ipm_solve_params_kernel<KIND, NX, NU, WPS, RESUME, XLDS>), dim3(grid), dim3(64), lds, s,
                       p, w, tp, mode, terminal, bp0, max_solves);
    return hipGetLastError();
  }
  // the structure-aware blocks unless NOC_PERSIST_STRUCT=0 (per launch: tests switch it)
  const char* senv = getenv("NOC_PERSIST_STRUCT");
  if (senv && atoi(senv) == 0)
    hipLaunchKernelGGL((ipm_solve_kernel<KIND, NX, NU, WPS, RESUME, XLDS, false>), dim3(grid), dim3(64),
                       lds, s, p, w, mode, terminal, bp0, max_solves);
  else
    hipLaunchKernelGGL((ipm_solve_kernel<KIND, NX, NU, WPS, RESUME, XLDS, true>), dim3(grid), dim3(64),
                       lds, s, p, w, mode, terminal, bp0, max_solves);
  return hipGetLastError();
}

// Speculative retries (SPEC waves per trajectory, the one-wave-per-SIMD register budget): when
// the batch leaves SIMDs idle, a trajectory's workgroup runs SPEC waves on SPEC SIMDs, wave k
// solving the KKT system and the trial of the k-th candidate of the regularisation's failure chain
// (rp, rp r_inc, rp r_inc 2 r_inc, ...; P:167-173) at the same point; the accept tests are then
// replayed in solve order (ipm_solve_kernel), so counters and iterates are the one-wave solver's
// bit for bit.  A rejected trial no longer costs a KKT solve on the trajectory's serial chain:
// the heaviest of 512 cart-poles, 492 computed solves, takes 345 rounds at two candidates, 266 at
// four (tools/spec_estimate.py).  Needs x, u in LDS per wave.
// NOC_PERSIST_SPEC=1|2|4 overrides the choice.
static size_t spec_lds_rt(int nx, int nu, int N, int spec) {  // = xlds_off(N, spec, 0) + spec x, u
  const long long slots = ((long long)N * nu * (nx + 1) + nx + 1) & ~1LL;
  const long long xu = ((long long)(N + 1) * nx + (long long)N * nu + 1) & ~1LL;
  return (size_t)(spec * (slots + state_doubles() + xu) + specio_doubles(spec)) * sizeof(double);
}
template <int KIND, int NX, int NU>
static size_t spec_lds_bytes(int N, int spec) {
  return (size_t)(xlds_off<NX, NU>(N, spec, 0) + spec * xlds_doubles<NX, NU>(N)) * sizeof(double);
}
// Candidates per trajectory for this launch: 4 when four waves per trajectory still leave a SIMD
// each (B <= #SIMDs / 4), else 2 (B <= #SIMDs / 2), else 1; 1 for an ordered launch (its grid is
// the whole batch, most of it done), and when x, u of every wave do not fit 40 KB of LDS per wave.
// A resume may run them (the tail of a large batch, gathered: BatchedIPM.solve_persistent).  The
// families with a one-wave instance only (cart-pole).  NOC_PERSIST_SPEC=1|2|4 forces it.
static int spec_auto(const noc_family& p, const noc_ipm_ws& w, int simds, bool launch_state) {
  if (p.kind != NOC_FAMILY_CARTPOLE) return 1;
  if (launch_state && w.order) return 1;
  const char* senv = getenv("NOC_PERSIST_STRUCT");
  if (senv && atoi(senv) == 0) return 1;
  const char* env = getenv("NOC_PERSIST_SPEC");  // per launch (A/B sweeps in one process)
  int want;
  if (env) {
    want = atoi(env);
  } else if (simds <= 0) {
    want = 1;
  } else {
    want = (long long)w.Bt * 4 <= simds ? 4 : ((long long)w.Bt * 2 <= simds ? 2 : 1);
  }
  if (want != 2 && want != 4) return 1;
  return spec_lds_rt(p.nx, p.nu, w.N, want) <= (size_t)want * 40960u ? want : 1;
}
// grid: workgroups = the entries of w.order this launch solves (w.Bt without an order)
template <int KIND, int NX, int NU, int SPEC>
static hipError_t launch_spec(const noc_family& p, const noc_ipm_ws& w, int mode, int terminal,
                              double bp0, int max_solves, hipStream_t s, int grid = -1) {
  if (grid < 0) grid = w.Bt;
  const size_t lds = spec_lds_bytes<KIND, NX, NU>(w.N, SPEC);
  if (w.flags & NOC_WS_RESUME)
    hipLaunchKernelGGL((ipm_solve_kernel<KIND, NX, NU, 1, true, true, true, SPEC>), dim3(grid), dim3(64 * SPEC),
                       lds, s, p, w, mode, terminal, bp0, max_solves);
  else
    hipLaunchKernelGGL((ipm_solve_kernel<KIND, NX, NU, 1, false, true, true, SPEC>), dim3(grid), dim3(64 * SPEC),
                       lds, s, p, w, mode, terminal, bp0, max_solves);
  return hipGetLastError();
}

template <int KIND, int NX, int NU, int WPS>
static hipError_t solve_w(const noc_family& p, const noc_ipm_ws& w, int mode, int terminal,
                          double bp0, int max_solves, size_t lds, hipStream_t s, int grid = -1,
                          const double* tp = nullptr) {
  if (grid < 0) grid = w.Bt;
  // x, u in LDS (XLDS) when that keeps the residency the register budget allows: 8 waves per CU
  // at 2 waves per SIMD (<= 20 KB per wave), 4 at one wave per SIMD (<= 40 KB); longer horizons
  // keep them in the workspace.  NOC_PERSIST_XLDS=0 forces the workspace (A/B).
  const char* xenv = getenv("NOC_PERSIST_XLDS");  // per launch (tests switch it)
  const size_t xl = lds + (size_t)(((w.N + 1) * NX + w.N * NU + 1) & ~1) * sizeof(double);
  const bool xlds = !(xenv && atoi(xenv) == 0) && xl <= (WPS == 1 ? 40960u : 20480u);
  const bool res = (w.flags & NOC_WS_RESUME) != 0;
  if (xlds)
    return res ? launch_solve<KIND, NX, NU, WPS, true, true>(p, w, mode, terminal, bp0, max_solves, xl, s, grid, tp)
               : launch_solve<KIND, NX, NU, WPS, false, true>(p, w, mode, terminal, bp0, max_solves, xl, s, grid, tp);
  return res ? launch_solve<KIND, NX, NU, WPS, true, false>(p, w, mode, terminal, bp0, max_solves, lds, s, grid, tp)
             : launch_solve<KIND, NX, NU, WPS, false, false>(p, w, mode, terminal, bp0, max_solves, lds, s, grid, tp);
}

// Heavy-first split of an ordered launch larger than one wave per SIMD (cart-pole): the first
// `heavy` entries of w.order -- the costliest trajectories (the probe-ordered resume,
// BatchedIPM.solve_persistent) -- run on the one-wave instance, a SIMD of their own, concurrently
// with the rest on the two-wave instance (second stream, event fork / join).  Every trajectory's
// result is the same on either instance (tested).  NOC_PERSIST_HEAVY=<n> sets the count.
// By default (cart-pole, N <= 320, #SIMDs < B <= 2 #SIMDs: the c3 slice of 2 GPUs) the costliest
// #SIMDs / 8 trajectories of the probe order run two speculative candidates each beside the rest
// on the two-wave instance: 2048 cart-poles 17.9 -> 16.3-16.8 ms (probe order alone;
// profiles/r06/t/).  At one wave per SIMD (1024) the split made the light end of the order wait
// for SIMDs: 11.4-11.6 ms on one batch but 16.2-18.5 ms on the c3 slices (profiles/r06/final_c4/),
// so not there; at c3 (4096) it measured slower (profiles/r06/q/).  NOC_PERSIST_HEAVY=<n> sets
// the count, NOC_PERSIST_HEAVY_SPEC=0|2 the candidates (0 turns the default split off).
static int heavy_count(const noc_ipm_ws& w, int simds, bool* spec2) {
  const char* env = getenv("NOC_PERSIST_HEAVY");  // per launch (A/B sweeps in one process)
  const char* hs = getenv("NOC_PERSIST_HEAVY_SPEC");
  *spec2 = false;
  if (!w.order || simds <= 0) return 0;
  // the candidates exist on the structure-aware blocks only (launch_spec), and both launches of a
  // split write the same w.A ... w.M: under NOC_PERSIST_STRUCT=0 no candidates (as spec_auto), so
  // the heavy launch takes the dense one-wave instance like the rest, or there is no split
  const char* senv = getenv("NOC_PERSIST_STRUCT");
  const bool dense = senv && atoi(senv) == 0;
  int h;
  bool sp;
  if (env) {
    h = atoi(env);
    sp = hs && atoi(hs) == 2 && !dense;
    if (w.Bt <= (sp ? simds / 2 : simds)) return 0;
  } else {
    if (dense || (hs && atoi(hs) == 0) || w.N > 320 || w.Bt <= simds || w.Bt > 2 * simds) return 0;
    h = simds / 8;
    sp = true;
  }
  if (h < 0) h = 0;
  if (h > simds / 2) h = simds / 2;
  *spec2 = sp;
  return h < w.Bt ? h : 0;
}

template <int KIND, int NX, int NU, int REST_WPS = 2>
static hipError_t solve_split(const noc_family& p, const noc_ipm_ws& w, int mode, int terminal,
                              double bp0, int max_solves, size_t lds, hipStream_t s, int heavy,
                              bool spec2) {
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
  // the heavy launch first, so its workgroups are placed before the two-wave ones fill the SIMDs;
  // spec2: the heavy trajectories with two speculative candidates each
  if (spec2 && spec_lds_bytes<KIND, NX, NU>(w.N, 2) <= 2 * 40960u)
    e = launch_spec<KIND, NX, NU, 2>(p, w, mode, terminal, bp0, max_solves, s, heavy);
  else
    e = solve_w<KIND, NX, NU, 1>(p, w, mode, terminal, bp0, max_solves, lds, s, heavy);
  if (e != hipSuccess) return e;
  noc_ipm_ws rest = w;
  rest.order = w.order + heavy;
  if ((e = solve_w<KIND, NX, NU, REST_WPS>(p, rest, mode, terminal, bp0, max_solves, lds, s2, w.Bt - heavy)) !=
      hipSuccess)
    return e;
  if ((e = hipEventRecord(join, s2)) != hipSuccess) return e;
  return hipStreamWaitEvent(s, join, 0);
}

template <int KIND, int NX, int NU>
static hipError_t solve_t(const noc_family& p, const noc_ipm_ws& w, int mode, int terminal,
                          double bp0, int max_solves, hipStream_t s) {
  const size_t lds = solve_lds_bytes(NX, NU, w.N);
  if (lds == 0) return hipErrorInvalidValue;  // step does not fit in LDS: use the launch driver
  if constexpr (one_wave_instance<KIND>()) {
    static const int simds = device_simds();
    static const char* env = getenv("NOC_PERSIST_WAVES");
    const bool one = env ? atoi(env) == 1 : (simds > 0 && w.Bt <= simds);
    if (one) {
      bool sp1 = false;
      const int heavy1 = env ? 0 : heavy_count(w, simds, &sp1);
      if (heavy1 > 0)
        return solve_split<KIND, NX, NU, 1>(p, w, mode, terminal, bp0, max_solves, lds, s, heavy1, sp1);
      const int spec = spec_auto(p, w, simds, true);
      if (spec == 2) return launch_spec<KIND, NX, NU, 2>(p, w, mode, terminal, bp0, max_solves, s);
      if (spec == 4) return launch_spec<KIND, NX, NU, 4>(p, w, mode, terminal, bp0, max_solves, s);
      return solve_w<KIND, NX, NU, 1>(p, w, mode, terminal, bp0, max_solves, lds, s);
    }
    bool sp = false;
    const int heavy = env ? 0 : heavy_count(w, simds, &sp);
    if (heavy > 0) return solve_split<KIND, NX, NU>(p, w, mode, terminal, bp0, max_solves, lds, s, heavy, sp);
  }
  return solve_w<KIND, NX, NU, 2>(p, w, mode, terminal, bp0, max_solves, lds, s);
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

// persistent instances exist for the families with nx <= 4 (an nx = 8 scan element does not fit a
// wave's registers next to the solver state: those run the launch-per-phase driver)
template <int NX>
constexpr bool persistent_instance() { return NX <= 4; }

bool ipm_solve_supported(const noc_family& p, int N, int lanes) {
  if (lanes != PL) return false;
  return for_family(p, false, [](auto, auto X, auto) { return persistent_instance<X>(); }) &&
         solve_lds_bytes(p.nx, p.nu, N) > 0;
}

// The wide kernel (ipm_wide.hip: 4 waves and the LDS of one CU per trajectory) when the batch
// leaves CUs idle anyway (B <= #CUs: the reference's B = 1 runs) and the horizon gives the
// one-wave kernel more than two stages per lane: at N <= 128 the one-wave solve is faster (its
// KKT scan needs no cross-wave join), beyond it the wide one (B = 1, per KKT solve: pendulum
// N=200 16.5 vs 20.4 us, N=800 32 vs 57 us; cart-pole N=128 31.6 vs 25.7 us, N=200 33.0 vs
// 35.2 us -- profiles/r02/wide/crossover.jsonl).  NOC_PERSIST_WIDE=0|1 overrides.
// (Re-packing the last <= #CUs trajectories of a large batch onto it was measured and dropped:
// those are Newton retries, KKT-bound, and the wide KKT solve is no faster -- DESIGN.md §3.7.)
// Where the speculative candidates apply (cart-pole, B <= #SIMDs / 2) and the horizon gives the
// one-wave kernel at most five stages per lane (N <= 320), they beat the wide kernel: cart-pole
// B = 1 N = 200 / 300 5.19 / 5.92 ms against 5.88 / 6.32 ms, N = 200 B = 64 / 256 7.54 / 8.30 ms
// against 9.53 / 10.28 ms; at N = 400 the wide kernel is ahead (6.57 vs 7.02 ms;
// profiles/r06/n/).  The choice ignores resume and order, so a capped solve resumes on the kernel
// family (one-wave) it started on.
static bool use_wide(const noc_family& p, const noc_ipm_ws& w) {
  const char* env = getenv("NOC_PERSIST_WIDE");
  if (env && atoi(env) == 0) return false;
  if (!ipm_wide_supported(p, w.N)) return false;
  if (env && atoi(env) == 1) return true;
  static const int simds = device_simds();
  const int cus = simds / 4;
  if (w.N <= 320 && spec_auto(p, w, simds, false) > 1) return false;
  return cus > 0 && w.Bt <= cus && w.N > 128;
}

hipError_t ipm_solve(const noc_family& p, const noc_ipm_ws& w, int mode, int terminal, double bp0,
                     int max_solves, hipStream_t s) {
  if (use_wide(p, w)) {
    static const int cus = device_simds() / 4;
    return ipm_solve_wide(p, w, mode, terminal, bp0, max_solves, nullptr, nullptr, w.Bt,
                          wide_waves(p, w, cus), s);
  }
  return for_family(p, hipErrorInvalidValue, [&](auto K, auto X, auto U) {
    if constexpr (persistent_instance<X>()) return solve_t<K, X, U>(p, w, mode, terminal, bp0, max_solves, s);
    else return hipErrorInvalidValue;
  });
}

// Per-trajectory cost parameters (noc_ipm_solve_params): always the one-wave kernel, with the
// register budget (one or two waves per SIMD) and the x, u placement solve_t / solve_w choose for
// the same batch -- never the wide kernel, speculative candidates or the heavy-first split, whose
// instances read the shared family argument.
hipError_t ipm_solve_params(const noc_family& p, const noc_ipm_ws& w, const double* tp, int mode,
                            int terminal, double bp0, int max_solves, hipStream_t s) {
  return for_family(p, hipErrorInvalidValue, [&](auto K, auto X, auto U) {
    if constexpr (persistent_instance<X>() && traj_params_instance<K, X, U>()) {
      const size_t lds = solve_lds_bytes(X, U, w.N);
      if (lds == 0) return hipErrorInvalidValue;
      if constexpr (one_wave_instance<K>()) {
        static const int simds = device_simds();
        static const char* env = getenv("NOC_PERSIST_WAVES");
        if (env ? atoi(env) == 1 : (simds > 0 && w.Bt <= simds))
          return solve_w<K, X, U, 1>(p, w, mode, terminal, bp0, max_solves, lds, s, -1, tp);
      }
      return solve_w<K, X, U, 2>(p, w, mode, terminal, bp0, max_solves, lds, s, -1, tp);
    } else {
      return hipErrorInvalidValue;
    }
  });
}

}  // namespace noc
