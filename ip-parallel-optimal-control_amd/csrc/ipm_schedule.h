// The interior-point solvers' Newton accept rule and barrier schedule, written once: the solver
// state of one trajectory, the accept step on it (gain ratio, rp / r_inc update, retry accounting,
// Newton stop test, barrier stage finish: P:159-245 / S:126-187), the point a later launch resumes
// at, and the regularisation a KKT solve is fed.  Included by the launch-per-phase trial kernel
// (ipm_kernels.hip) and the one-wave and wide persistent kernels (ipm_persistent.hip,
// ipm_wide.hip), which therefore take identical decisions on identical inputs, and by the DDP
// kernel (ddp_persistent.hip), whose own rule (D:126-152) shares the barrier step and, from
// noc_internal.h, the clip, the retry cap and the retry accounting.
// Wave-uniform scalar code with no multiply feeding an add outside rp_shrink (which turns
// contraction off), so -ffp-contract cannot change a bit of it.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/noc_hip.h"
#include "noc_internal.h"
#include "small_linalg.h"

namespace noc {

NOC_DEV double next_barrier(double bp) { return bp / 5.0; }  // P:238 / S:186 / D:195

// rp and r_inc after one trial (P:167-173 / S:139-144; shrink: rp_shrink(gain)); the clip is par's
NOC_DEV void reg_update(int mode, bool success, double shrink, double& rp, double& rinc) {
  rp = success ? rp * shrink : rp * rinc;
  rinc = success ? 2.0 : 2.0 * rinc;
  if (mode == NOC_MODE_PAR) rp = rp_clip(rp);
}

// The regularisation fed to the KKT solve: par R += rp*||cu||*I (P:116-118); seq Quu += mu*I (S:51)
NOC_DEV double candidate_reg(int mode, double rp, double gnorm) {
  return (mode == NOC_MODE_PAR) ? rp * gnorm : rp;
}

// The phase a persistent solve resumes at (NOC_WS_RESUME) from a workspace phase, including the
// two-stream driver's intermediate ones: ROLLED (states current) continues with a new Newton
// iteration, ROLLOUT_PENDING with the rollout.
NOC_DEV int resume_phase(int ph) {
  if (ph == NOC_PHASE_ROLLED) return NOC_PHASE_LINEARIZE;
  if (ph == NOC_PHASE_ROLLOUT_PENDING) return NOC_PHASE_ROLLOUT;
  return ph;
}

// The hand-off marker.  A persistent launch that stops at its solve cap leaves kkt_active = 0
// (IpmState::store), while the launch-per-phase driver never leaves a SOLVE trajectory without
// kkt_active = 1 (mark_solve_kernel; the trial kernel does not touch it).  So (SOLVE,
// kkt_active == 0) says "this trajectory's LQ blocks, cx, cu, lam, r, P and reg are not in this
// workspace": the launch-per-phase prepare rebuilds them from x, u, bp, rp, gnorm before its
// KKT scan reads them (ipm_kernels.hip), leaving it, inner, cost, hu and gnorm as they are.
NOC_DEV bool blocks_missing(const noc_ipm_ws& w, int b, int ph) {
  return ph == NOC_PHASE_SOLVE && w.kkt_active[b] == 0;
}
// The trajectories a launch-per-phase prepare builds blocks for: a new Newton iteration, or a
// retry that a persistent launch handed over
NOC_DEV bool builds_blocks(const noc_ipm_ws& w, int b) {
  const int ph = w.phase[b];
  return ph == NOC_PHASE_LINEARIZE || blocks_missing(w, b, ph);
}

// Where the solve continues after an accept step: the next barrier stage's rollout (P:243-245;
// NOC_WS_ONE_STAGE: newton_oc runs a single stage), a new linearisation, or a retry on the same
// blocks with the new regularisation
NOC_DEV int resume_point(bool stage_done, bool relinearize, double bp, int flags) {
  if (stage_done) return (bp > 1e-4 && !(flags & NOC_WS_ONE_STAGE)) ? NOC_PHASE_ROLLOUT : NOC_PHASE_DONE;
  return relinearize ? NOC_PHASE_LINEARIZE : NOC_PHASE_SOLVE;
}

// Wave-uniform solver state of one trajectory: the workspace's per-trajectory fields
struct IpmState {
  double bp, rp, rinc, cost, hu, gnorm;
  int it, inner, total_it, solves;
  NOC_DEV void init(double bp0) {
    bp = bp0; rp = 1.0; rinc = 2.0; cost = 0.0; hu = 1.0; gnorm = 0.0;
    it = 0; inner = 0; total_it = 0; solves = 0;
  }
  NOC_DEV void load(const noc_ipm_ws& w, int b) {
    bp = w.bp[b]; rp = w.rp[b]; rinc = w.rinc[b]; cost = w.cost[b]; hu = w.hu[b];
    gnorm = w.gnorm[b]; it = w.it[b]; inner = w.inner[b]; total_it = w.total_it[b];
    solves = w.kkt_solves[b];
  }
  // the end of a persistent launch: `phase` is DONE or where a later launch continues
  NOC_DEV void store(const noc_ipm_ws& w, int b, int phase) const {
    w.bp[b] = bp; w.rp[b] = rp; w.rinc[b] = rinc; w.cost[b] = cost; w.hu[b] = hu;
    w.gnorm[b] = gnorm; w.it[b] = it; w.inner[b] = inner; w.total_it[b] = total_it;
    w.kkt_solves[b] = solves;
    w.kkt_active[b] = 0;
    w.phase[b] = phase;
  }
};

struct AcceptOutcome {
  double gain;
  int rep;           // identical retries accounted for without a solve (counted in inner, solves)
  bool success;
  bool take;         // x <- x + dx, u <- u + du
  bool end_iter;     // the Newton iteration ended
  bool stage_done;   // ... and the stop test ended the barrier stage (bp, it, rp, r_inc advanced)
  bool relinearize;  // the next solve needs new blocks (false: a retry, only reg changes)
};

// One accept test (P:159-202 / S:126-161) and, when it ends the barrier stage, the stage finish
// (P:238-239 / S:186-187) on the solver state.  new_cost: the trial's total cost, inf when
// infeasible; pred, bwd_ok: the KKT solve's predicted decrease and backward feasibility; flags:
// the workspace's; room: how many accounted retries the caller's solve cap still allows.
// trace, b: the caller's decision-trace global and trajectory (NOC_DECISION_TRACE builds).
NOC_DEV AcceptOutcome accept_step(IpmState& s, int mode, double new_cost, double pred, bool bwd_ok,
                                  int flags, int room, const DecisionTrace* trace = nullptr,
                                  int b = 0) {
  AcceptOutcome o;
  o.gain = (new_cost - s.cost) / pred;                        // P:164-165
  o.success = (o.gain > 0.0) && bwd_ok;                       // P:166 / S:137
#ifdef NOC_DECISION_TRACE
  if (trace) NOC_TRACE_DECISION(*trace, b, s.solves, s.bp, s.it, s.inner, s.cost, new_cost, pred,
                                o.gain, o.success, s.rp, s.rinc, s.hu, bwd_ok);
#endif
  const double rp_used = s.rp;
  reg_update(mode, o.success, rp_shrink(o.gain), s.rp, s.rinc);
  s.inner += 1;
  o.rep = 0;
  if (mode == NOC_MODE_PAR) {
    // identical retries at the rp clip: accounted, not recomputed (noc_internal.h)
    o.rep = par_retry_repeats(flags, o.success, rp_used, s.rp, s.inner, room);
    s.inner += o.rep;
    s.solves += o.rep;
    s.rinc = ldexp(s.rinc, o.rep);                            // r_inc doubles per retry (P:172)
    o.end_iter = o.success || retry_cap_reached(s.inner);
    o.take = o.end_iter;                                      // the last trial is kept (P:175, P:184)
    o.stage_done = o.end_iter && (s.hu < 1e-4 || s.it + 1 > 1000);  // P:199-202
  } else {
    o.take = o.success;                                       // S:145-146
    o.end_iter = true;
    o.stage_done = (s.hu < 1e-4) && bwd_ok;                   // S:157-161
  }
  s.solves += 1;
  s.it += o.end_iter ? 1 : 0;
  o.relinearize = false;
  if (o.stage_done) {
    s.total_it += s.it;                                       // P:239 / S:187
    s.bp = next_barrier(s.bp);
    s.it = 0;
    s.rp = 1.0;                                               // P:134 / S:110
    s.rinc = 2.0;                                             // P:135 / S:111
  } else if (mode == NOC_MODE_PAR) {
    o.relinearize = o.end_iter;
  } else {
    // seq: a rejected step leaves x, u unchanged, so only the regularisation changes (same
    // blocks, cheaper: skip relinearising)
    o.relinearize = o.success;
  }
  return o;
}

}  // namespace noc
