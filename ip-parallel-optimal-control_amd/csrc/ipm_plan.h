// What one noc_ipm_solve / noc_ipm_solve_params call launches (ipm_persistent.hip, ipm_wide.hip):
// the environment switches (PersistKnobs), the LDS sizes of the one-wave kernel's instances, and
// the decision itself (plan_persist) as a pure function of the batch, the device's SIMD count and
// the switches.  Host logic only -- no device code, no HIP call: the launcher consumes a
// PersistPlan, noc_debug_ipm_plan reports one, tests/test_ipm_plan.py pins the table.
#pragma once
#include <climits>
#include <cstddef>
#include <cstdlib>

#include "../../include/noc_hip.h"

#ifdef __HIPCC__
#define NOC_HOST_DEV __host__ __device__
#else
#define NOC_HOST_DEV
#endif

namespace noc {

// ---- LDS of one one-wave-kernel workgroup, in doubles (the kernels index with these, the plan
// sizes the launch with them; I = int in the kernels, long long on the host: any N the ABI lets
// through is sized without overflow).  SPEC regions of KKT slots (kkt_scan_impl.h lds_slots: one
// per 64-lane segment), SPEC parked states, SPEC SpecIO records (SPEC > 1 only), then SPEC copies
// of x, u (XLDS).  SPEC = 1 is the one-wave layout: [slots][state][x, u].
constexpr int kIpmStateBytes = 64;  // sizeof(IpmState) (ipm_schedule.h), asserted where it is parked
constexpr int kSpecIOBytes = 48;    // sizeof(SpecIO) (ipm_persistent.hip), asserted there
template <class I>
NOC_HOST_DEV constexpr I slot_doubles(int nx, int nu, I N) { return (N * (nu * (nx + 1)) + nx + 1) & ~(I)1; }
NOC_HOST_DEV constexpr int state_doubles() { return (kIpmStateBytes + 15) / 16 * 2; }
NOC_HOST_DEV constexpr int specio_doubles(int spec) { return spec > 1 ? kSpecIOBytes / 8 * spec : 0; }
// XLDS: x [(N+1) nx], u [N nu] of the trajectory behind the slots and the parked state
template <class I>
NOC_HOST_DEV constexpr I xlds_doubles(int nx, int nu, I N) { return ((N + 1) * nx + N * nu + 1) & ~(I)1; }
template <class I>
NOC_HOST_DEV constexpr I xlds_off(int nx, int nu, I N, int spec = 1, int wv = 0) {
  return spec * (slot_doubles(nx, nu, N) + state_doubles()) + specio_doubles(spec) + wv * xlds_doubles(nx, nu, N);
}
// Launch sizes in bytes.  One wave per trajectory: the KKT slots + the parked state (+ 16), 0
// beyond 64 KB (long horizons at small batch, e.g. the reference's N = 1000 timing runs: 2
// workgroups per CU) -- the step does not fit in LDS: use the launch driver; xlds adds x, u.
constexpr long long onewave_lds_bytes(int nx, int nu, long long N) {
  const long long bytes = slot_doubles(nx, nu, N) * 8 + kIpmStateBytes + 16;
  return bytes <= 65536 ? bytes : 0;
}
constexpr long long spec_lds_bytes(int nx, int nu, long long N, int spec) {
  return (xlds_off(nx, nu, N, spec, 0) + spec * xlds_doubles(nx, nu, N)) * 8;
}

// Families whose kernel spills at 2 waves per SIMD (cart-pole) get a second instance at 1 wave per
// SIMD (512 registers per lane: no scratch, stage pairs), used when the batch fits one wave per
// SIMD anyway (B <= 4 x CUs: the reference's B = 1 runs, c2-sized batches); larger batches keep 2
// waves per SIMD for latency hiding.  The others stay at 2 waves (their 1-wave instance measured
// 5-7 % slower at B = 1).
constexpr bool one_wave_instance(int kind) { return kind == NOC_FAMILY_CARTPOLE; }
// persistent instances exist for the families with nx <= 4 (an nx = 8 scan element does not fit a
// wave's registers next to the solver state: those run the launch-per-phase driver)
constexpr bool persistent_instance(int nx) { return nx <= 4; }

// ---- the environment switches of the persistent solver: the single list ----
struct PersistKnobs {
  static constexpr int kUnset = INT_MIN;  // the variable is not in the environment
  // NOC_PERSIST_WIDE=0|1: never / always (where it fits) the wide kernel instead of the rule in
  // plan_persist.
  int wide = kUnset;
  // NOC_PERSIST_WAVES=1|2: the one-wave kernel's register budget (waves per SIMD; 1 only for
  // families with one_wave_instance) instead of "1 while B <= #SIMDs" (timing experiments).  Set to
  // anything, it also turns the heavy-first split off.  The only one read once per process.
  int waves = kUnset;
  // NOC_PERSIST_SPEC=1|2|4: the speculative candidates per trajectory instead of the rule in
  // plan_spec (still within its LDS cap, and not on an ordered launch).
  int spec = kUnset;
  // NOC_PERSIST_STRUCT=0: the dense-block instance, which computes the same doubles as the
  // structure-aware one (block_struct.h).  The candidates exist on the structure-aware blocks
  // only, and both launches of a split write the same w.A ... w.M: so no candidates, and a forced
  // split's heavy launch takes the dense one-wave instance like the rest.
  int strct = kUnset;
  // NOC_PERSIST_XLDS=0: x, u stay in the workspace whatever the LDS cap allows (A/B).
  int xlds = kUnset;
  // NOC_PERSIST_HEAVY=<n>: the heavy-first split with n trajectories (at most #SIMDs / 2) in its
  // heavy launch, for any family with a one-wave instance, horizon and batch above the bounds in
  // plan_heavy.
  int heavy = kUnset;
  // NOC_PERSIST_HEAVY_SPEC=0|2: the candidates of the heavy launch; 0 turns the default split
  // off, 2 gives a forced split (NOC_PERSIST_HEAVY) candidates.
  int heavy_spec = kUnset;
  // NOC_WIDE_WAVES=2|4: waves per trajectory of the wide kernel instead of the rule in
  // plan_persist.
  int wide_waves = kUnset;

  bool dense() const { return strct == 0; }
};

inline int env_int(const char* name, int unset) {
  const char* e = std::getenv(name);
  return e ? std::atoi(e) : unset;
}

// The only getenv site of these names.  All but NOC_PERSIST_WAVES are read at every launch: tests
// and A/B sweeps switch them inside one process.
inline PersistKnobs read_persist_knobs() {
  static const int waves = env_int("NOC_PERSIST_WAVES", PersistKnobs::kUnset);
  PersistKnobs k;
  k.wide = env_int("NOC_PERSIST_WIDE", k.kUnset);
  k.waves = waves;
  k.spec = env_int("NOC_PERSIST_SPEC", k.kUnset);
  k.strct = env_int("NOC_PERSIST_STRUCT", k.kUnset);
  k.xlds = env_int("NOC_PERSIST_XLDS", k.kUnset);
  k.heavy = env_int("NOC_PERSIST_HEAVY", k.kUnset);
  k.heavy_spec = env_int("NOC_PERSIST_HEAVY_SPEC", k.kUnset);
  k.wide_waves = env_int("NOC_WIDE_WAVES", k.kUnset);
  return k;
}

// ---- the plan ----
// One launch of the one-wave kernel family: the template arguments of its instance
// (ipm_persistent.hip: ipm_solve_kernel), `grid` workgroups of 64 * spec threads -- the entries of
// w.order this launch solves (w.Bt without an order) -- and the dynamic LDS.
struct PersistLaunch {
  int wps = 2;          // waves per SIMD the register budget is sized for
  int spec = 1;         // waves per trajectory (speculative candidates); > 1: wps 1, xlds, strct
  bool resume = false;  // NOC_WS_RESUME
  bool xlds = false;    // x, u in LDS for the whole solve
  bool strct = true;    // structure-aware blocks
  int grid = 0;
  long long lds = 0;    // bytes
};
struct PersistPlan {
  enum Family { kNone = 0, kOneWave = 1, kWide = 2 };
  Family family = kNone;  // kNone: no persistent instance (nx > 4) or the step does not fit in LDS
  // kWide (ipm_wide.hip): one workgroup of wide_waves waves per trajectory, grid = Bt
  int wide_waves = 0;
  long long wide_lds = 0;
  // kOneWave: the launch -- or, with heavy > 0, the heavy-first split: `main` solves the first
  // `heavy` entries of w.order (spec 2 on compact blocks, or the plain one-wave-per-SIMD
  // instance), concurrently with `rest` on the others
  PersistLaunch main, rest;
  int heavy = 0;
};

// What plan_persist decides from.  simds: SIMDs of the device (4 per CU), 0 if unknown.
// wide_lds2 / wide_lds4: LDS bytes of the wide kernel's workgroup at 2 / 4 waves, 0 where the wide
// kernel does not cover (family, N) (WideLds lives in device headers: ipm_wide.hip).
struct PersistQuery {
  int kind, nx, nu, N, Bt;
  bool ordered;      // w.order present
  int flags;         // NOC_WS_* bits of the workspace
  bool with_params;  // noc_ipm_solve_params: per-trajectory records
  int simds;
  long long wide_lds2, wide_lds4;
};

// Speculative retries (SPEC waves per trajectory, the one-wave-per-SIMD register budget): when
// the batch leaves SIMDs idle, a trajectory's workgroup runs SPEC waves on SPEC SIMDs, wave k
// solving the KKT system and the trial of the k-th candidate of the regularisation's failure chain
// (rp, rp r_inc, rp r_inc 2 r_inc, ...; P:167-173) at the same point; the accept tests are then
// replayed in solve order (ipm_solve_kernel), so counters and iterates are the one-wave solver's
// bit for bit.  A rejected trial no longer costs a KKT solve on the trajectory's serial chain:
// the heaviest of 512 cart-poles, 492 computed solves, takes 345 rounds at two candidates, 266 at
// four (tools/spec_estimate.py).  Needs x, u in LDS per wave.
// Candidates per trajectory for a launch: 4 when four waves per trajectory still leave a SIMD
// each (B <= #SIMDs / 4), else 2 (B <= #SIMDs / 2), else 1; 1 for an ordered launch (its grid is
// the whole batch, most of it done), and when x, u of every wave do not fit 40 KB of LDS per wave.
// A resume may run them (the tail of a large batch, gathered: BatchedIPM.solve_persistent).  The
// families with a one-wave instance only (cart-pole).  launch_state = false: the candidate rule
// as the wide-kernel choice consults it, whatever the order.
inline int plan_spec(const PersistQuery& q, const PersistKnobs& k, bool launch_state) {
  if (!one_wave_instance(q.kind)) return 1;
  if (launch_state && q.ordered) return 1;
  if (k.dense()) return 1;
  int want;
  if (k.spec != k.kUnset) {
    want = k.spec;
  } else if (q.simds <= 0) {
    want = 1;
  } else {
    want = (long long)q.Bt * 4 <= q.simds ? 4 : ((long long)q.Bt * 2 <= q.simds ? 2 : 1);
  }
  if (want != 2 && want != 4) return 1;
  return spec_lds_bytes(q.nx, q.nu, q.N, want) <= want * 40960LL ? want : 1;
}

// Heavy-first split of an ordered launch larger than one wave per SIMD (cart-pole): the first
// `heavy` entries of w.order -- the costliest trajectories (the probe-ordered resume,
// BatchedIPM.solve_persistent) -- run on the one-wave instance, a SIMD of their own, concurrently
// with the rest on the two-wave instance (second stream, event fork / join).  Every trajectory's
// result is the same on either instance (tested).
// By default (cart-pole, N <= 320, #SIMDs < B <= 2 #SIMDs: the c3 slice of 2 GPUs) the costliest
// #SIMDs / 8 trajectories of the probe order run two speculative candidates each beside the rest
// on the two-wave instance: 2048 cart-poles 17.9 -> 16.3-16.8 ms (probe order alone;
// profiles/r06/t/).  At one wave per SIMD (1024) the split made the light end of the order wait
// for SIMDs: 11.4-11.6 ms on one batch but 16.2-18.5 ms on the c3 slices (profiles/r06/final_c4/),
// so not there; at c3 (4096) it measured slower (profiles/r06/q/).  A forced count
// (NOC_PERSIST_HEAVY) has its own batch bound: B above #SIMDs, or above #SIMDs / 2 with candidates.
// Returns the heavy count (0: no split); *spec2: the heavy launch runs two candidates.
inline int plan_heavy(const PersistQuery& q, const PersistKnobs& k, bool* spec2) {
  *spec2 = false;
  if (!q.ordered || q.simds <= 0) return 0;
  int h;
  bool sp;
  if (k.heavy != k.kUnset) {
    h = k.heavy;
    sp = k.heavy_spec == 2 && !k.dense();
    if (q.Bt <= (sp ? q.simds / 2 : q.simds)) return 0;
  } else {
    if (k.dense() || k.heavy_spec == 0 || q.N > 320 || q.Bt <= q.simds || q.Bt > 2 * q.simds) return 0;
    h = q.simds / 8;
    sp = true;
  }
  if (h < 0) h = 0;
  if (h > q.simds / 2) h = q.simds / 2;
  *spec2 = sp;
  return h < q.Bt ? h : 0;
}

// One launch of `grid` workgroups at `wps` waves per SIMD, spec 1.  x, u in LDS (XLDS) when that
// keeps the residency the register budget allows: 8 waves per CU at 2 waves per SIMD (<= 20 KB
// per wave), 4 at one wave per SIMD (<= 40 KB); longer horizons keep them in the workspace.
inline PersistLaunch plan_launch(const PersistQuery& q, const PersistKnobs& k, int wps, int grid) {
  PersistLaunch l;
  l.wps = wps;
  l.resume = (q.flags & NOC_WS_RESUME) != 0;
  l.strct = q.with_params || !k.dense();  // the per-trajectory twin: the structure-aware instance only
  l.grid = grid;
  l.lds = onewave_lds_bytes(q.nx, q.nu, q.N);
  const long long xl = l.lds + xlds_doubles(q.nx, q.nu, (long long)q.N) * 8;
  l.xlds = k.xlds != 0 && xl <= (wps == 1 ? 40960 : 20480);
  if (l.xlds) l.lds = xl;
  return l;
}
// ... with `spec` > 1 candidates per trajectory: one wave per SIMD, x, u in LDS, compact blocks
inline PersistLaunch plan_spec_launch(const PersistQuery& q, int spec, int grid) {
  PersistLaunch l;
  l.wps = 1;
  l.spec = spec;
  l.resume = (q.flags & NOC_WS_RESUME) != 0;
  l.xlds = true;
  l.grid = grid;
  l.lds = spec_lds_bytes(q.nx, q.nu, q.N, spec);
  return l;
}

// The wide kernel (ipm_wide.hip: 4 waves and the LDS of one CU per trajectory) when the batch
// leaves CUs idle anyway (B <= #CUs: the reference's B = 1 runs) and the horizon gives the
// one-wave kernel more than two stages per lane: at N <= 128 the one-wave solve is faster (its
// KKT scan needs no cross-wave join), beyond it the wide one (B = 1, per KKT solve: pendulum
// N=200 16.5 vs 20.4 us, N=800 32 vs 57 us; cart-pole N=128 31.6 vs 25.7 us, N=200 33.0 vs
// 35.2 us -- profiles/r02/wide/crossover.jsonl).
// (Re-packing the last <= #CUs trajectories of a large batch onto it was measured and dropped:
// those are Newton retries, KKT-bound, and the wide KKT solve is no faster -- DESIGN.md §3.7.)
// Where the speculative candidates apply (cart-pole, B <= #SIMDs / 2) and the horizon gives the
// one-wave kernel at most five stages per lane (N <= 320), they beat the wide kernel: cart-pole
// B = 1 N = 200 / 300 5.19 / 5.92 ms against 5.88 / 6.32 ms, N = 200 B = 64 / 256 7.54 / 8.30 ms
// against 9.53 / 10.28 ms; at N = 400 the wide kernel is ahead (6.57 vs 7.02 ms;
// profiles/r06/n/).  The choice ignores resume and order, so a capped solve resumes on the kernel
// family (one-wave) it started on.
inline bool plan_wide(const PersistQuery& q, const PersistKnobs& k) {
  if (q.with_params || k.wide == 0 || q.wide_lds4 <= 0) return false;
  if (k.wide == 1) return true;
  const int cus = q.simds / 4;
  if (q.N <= 320 && plan_spec(q, k, false) > 1) return false;
  return cus > 0 && q.Bt <= cus && q.N > 128;
}

// Per-trajectory cost parameters (noc_ipm_solve_params) always get the one-wave kernel, with the
// register budget and the x, u placement of the same batch -- never the wide kernel, speculative
// candidates or the heavy-first split, whose instances read the shared family argument.
inline PersistPlan plan_persist(const PersistQuery& q, const PersistKnobs& k) {
  PersistPlan p;
  if (plan_wide(q, k)) {
    p.family = PersistPlan::kWide;
    // Waves per trajectory: 4 when the batch leaves CUs idle (B <= #CUs: one workgroup per CU), 2
    // when two two-wave workgroups fit a CU (512 registers per lane: one wave per SIMD) -- B up to
    // 2 x #CUs, the 8-GPU slice of c3.
    const int cus = q.simds / 4;
    if (k.wide_waves == 2 || k.wide_waves == 4) p.wide_waves = k.wide_waves;
    else if (cus > 0 && q.Bt <= cus) p.wide_waves = 4;
    else p.wide_waves = (q.wide_lds2 > 0 && q.wide_lds2 <= 80 * 1024 - 512) ? 2 : 4;
    p.wide_lds = p.wide_waves == 2 ? q.wide_lds2 : q.wide_lds4;
    return p;
  }
  if (!persistent_instance(q.nx) || onewave_lds_bytes(q.nx, q.nu, q.N) == 0) return p;
  p.family = PersistPlan::kOneWave;
  int wps = 2;
  if (one_wave_instance(q.kind)) {
    const bool forced = k.waves != k.kUnset;
    if (forced ? k.waves == 1 : (q.simds > 0 && q.Bt <= q.simds)) wps = 1;
    bool spec2 = false;
    p.heavy = (forced || q.with_params) ? 0 : plan_heavy(q, k, &spec2);
    if (p.heavy > 0) {  // the split: the rest keeps the batch's register budget
      p.main = (spec2 && spec_lds_bytes(q.nx, q.nu, q.N, 2) <= 2 * 40960)
                   ? plan_spec_launch(q, 2, p.heavy) : plan_launch(q, k, 1, p.heavy);
      p.rest = plan_launch(q, k, wps, q.Bt - p.heavy);
      return p;
    }
    const int spec = (wps == 1 && !q.with_params) ? plan_spec(q, k, true) : 1;
    if (spec > 1) {
      p.main = plan_spec_launch(q, spec, q.Bt);
      return p;
    }
  }
  p.main = plan_launch(q, k, wps, q.Bt);
  return p;
}

}  // namespace noc
