// extern "C" entry points of libnoc_hip.so (declared in include/noc_hip.h).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <string>

#include "../../include/noc_hip.h"
#include "noc_internal.h"
#include "small_linalg.h"

namespace noc {
static std::string kkt_shapes_str();
}

namespace {
thread_local std::string g_last_error;
int g_ablate = 0;  // timing-only phase ablation (noc_debug_set_ablation); never set in product use

int fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

// align: 16 where the kernels read / write the array with 16-byte vector accesses (the fp64 KKT
// fields), the natural alignment (8 for fp64, 4 for int32) elsewhere
int check_ptr(const void* p, const char* name, bool required, unsigned align = 16) {
  if (!p) return required ? fail(-2, std::string("required pointer is NULL: ") + name) : 0;
  if (reinterpret_cast<uintptr_t>(p) & (align - 1))
    return fail(-3, std::string("pointer not ") + std::to_string(align) + "-byte aligned: " + name);
  return 0;
}

int hip_status(hipError_t e, const char* where) {
  if (e == hipSuccess) return 0;
  return fail(-10, std::string(where) + ": " + hipGetErrorString(e));
}

// ---- the argument rules, each written once -------------------------------------------------------
struct Ptr {
  const void* p;
  const char* name;
  bool required;
  unsigned align = 16;
};

// in list order: the first offending pointer decides the code and the message
int check_ptrs(std::initializer_list<Ptr> list) {
  for (const Ptr& a : list)
    if (int rc = check_ptr(a.p, a.name, a.required, a.align)) return rc;
  return 0;
}

// ... every one required, under one name
int check_all(std::initializer_list<const void*> list, const char* name, unsigned align) {
  for (const void* p : list)
    if (int rc = check_ptr(p, name, true, align)) return rc;
  return 0;
}

// The _params and _compact forms report every argument error as -1 (include/noc_hip.h); a HIP
// error stays -10.
int args_as_minus1(int rc) { return rc < 0 && rc > -10 ? -1 : rc; }

bool lanes_in(int lanes, std::initializer_list<int> legal) {
  for (int l : legal)
    if (lanes == l) return true;
  return false;
}

int check_mode(int mode) {
  return mode == NOC_MODE_PAR || mode == NOC_MODE_SEQ ? 0 : fail(-1, "bad mode");
}

int check_terminal(int terminal) {
  return terminal == NOC_TERMINAL_FINAL_COST || terminal == NOC_TERMINAL_STAGE0
             ? 0 : fail(-1, "bad terminal option");
}

constexpr int kWsFlagsAll = NOC_WS_ONE_STAGE | NOC_WS_RESUME | NOC_WS_NO_REPEAT_SKIP;
int check_ws_flags(int flags, const std::string& what) {
  return flags & ~kWsFlagsAll ? fail(-1, what + " flags: unknown bits set (NOC_WS_ONE_STAGE | "
                                                "NOC_WS_RESUME | NOC_WS_NO_REPEAT_SKIP are defined)")
                              : 0;
}

int check_family(const noc_family* fam) {
  if (!fam) return fail(-2, "family is NULL");
  if (!noc::family_supported(*fam)) return fail(-1, "unsupported problem family (kind/nx/nu)");
  return 0;
}

int check_horizon_batch(int N, int B) {
  if (N < 1) return fail(-1, "horizon N must be >= 1");
  if (B < 0) return fail(-1, "batch B must be >= 0");
  return 0;
}

// the building blocks' sizes (N = 1 where the block has no horizon)
int check_block_dims(int N, int B) {
  return N < 1 || B < 0 ? fail(-1, "need N >= 1, B >= 0") : 0;
}

int check_dims(int nx, int nu, int N, int B, int lanes) {
  if (!noc::kkt_supported(nx, nu))
    return fail(-1, "unsupported (nx, nu) = (" + std::to_string(nx) + ", " + std::to_string(nu) +
                        "); supported: " + noc::kkt_shapes_str());
  if (int rc = check_horizon_batch(N, B)) return rc;
  if (!lanes_in(lanes, {0, 1, 8, 16, 32, 64, 128}))
    return fail(-1, "lanes must be 0, 1, 8, 16, 32, 64 or 128");
  return 0;
}
}  // namespace

namespace noc {
bool kkt_supported(int nx, int nu) {
#define NOC_KKT_SHAPE(X, U) if (nx == X && nu == U) return true;
#include NOC_KKT_SHAPES_DEF
#undef NOC_KKT_SHAPE
  return false;
}

static std::string kkt_shapes_str() {
  std::string s;
#define NOC_KKT_SHAPE(X, U) s += std::string(s.empty() ? "" : " ") + "(" #X "," #U ")";
#include NOC_KKT_SHAPES_DEF
#undef NOC_KKT_SHAPE
  return s;
}

hipError_t kkt_dispatch(int nx, int nu, const KKTArgs& a, int lanes, hipStream_t stream) {
  if (lanes == 1) return kkt_group_dispatch(nx, nu, a, stream);
#define NOC_KKT_SHAPE(X, U) if (nx == X && nu == U) return kkt_dispatch_shape<X, U>(a, lanes, stream);
#include NOC_KKT_SHAPES_DEF
#undef NOC_KKT_SHAPE
  return hipErrorInvalidValue;
}

// lanes per trajectory chosen from the measured sweep (profiles/r01/kkt_lanes_sweep_tiled.log):
// long horizons amortise the cross-lane scan over longer chunks (L = 32 at c3, N = 200); short
// horizons need the lanes for parallelism (L = 64 at c2, N = 100).
int kkt_default_lanes(int nx, int nu, int N) {
  (void)nu;
  // nx = 8: the horizon-sequential group solve (lanes 1) -- c4: 6.1 ms vs 47-55 ms for the scan,
  // whose nx = 8 element spills (profiles/r01/session2/r9_sweep_c4.log, bench_c4_dma.log)
  if (nx >= 8) return 1;
  return N >= 160 ? 32 : 64;
}


// Batch-aware lanes per trajectory (the measured lanes x horizon x batch sweep,
// profiles/r01/session4/lanes_policy/): (1) the longest-parallel split whose chunks still hold
// >= cmin stages (the cross-lane combine is amortised over the chunk: nx = 2 needs 3, nx = 4 four;
// shorter chunks are combine-bound, longer ones serialise the lane and, at L = 32 and N >= 300,
// the on-chip gains cap residency at 6 waves/CU), then (2) double L while the batch gives fewer
// waves than the device has SIMDs (a half-empty chip loses more than a short chunk costs), up to
// two waves per trajectory.
int kkt_pick_lanes(int nx, int nu, int N, int B) {
  if (nx >= 8) return kkt_default_lanes(nx, nu, N);
  const int cmin = nx <= 2 ? 3 : 4;
  int L = 8;
  for (int c = 64; c >= 8; c /= 2)
    if (N >= cmin * c) { L = c; break; }
  const long simds = device_simds(1024);
  // (3) two waves per trajectory (L = 128, nx <= 4) only when the horizon gives every lane of
  // both waves a stage and the whole batch is resident at once: that instance runs one wave per
  // SIMD (kkt_scan_kernel), so B * 2 waves must not exceed the SIMDs
  while ((long)B * L < 64 * simds &&
         (L < 64 || (L == 64 && nx <= 4 && N >= 128 && (long)B * 2 <= simds)))
    L *= 2;
  return L;
}
}  // namespace noc

// sha256 (16 hex digits) of the sources, from the Makefile (-DNOC_BUILD_HASH); include/noc_hip.h
#ifndef NOC_BUILD_HASH
#define NOC_BUILD_HASH "unknown"
#endif

extern "C" {

int noc_abi_version(void) { return NOC_ABI_VERSION; }
const char* noc_build_hash(void) { return NOC_BUILD_HASH; }
void noc_debug_set_ablation(int bits) { g_ablate = bits; }
const char* noc_last_error(void) { return g_last_error.c_str(); }
int noc_kkt_supported(int nx, int nu) { return noc::kkt_supported(nx, nu) ? 1 : 0; }
int noc_kkt_default_lanes(int nx, int nu, int N) { return noc::kkt_default_lanes(nx, nu, N); }
int noc_kkt_pick_lanes(int nx, int nu, int N, int B) {
  if (check_dims(nx, nu, N, B, 0)) return -1;
  return noc::kkt_pick_lanes(nx, nu, N, B);
}
int noc_kkt_gains_on_chip(int nx, int nu, int N, int lanes) {
  if (check_dims(nx, nu, N, 1, lanes)) return 0;
  const int L = lanes ? lanes : noc::kkt_default_lanes(nx, nu, N);
  return noc::kkt_lds_bytes_rt(nx, nu, N, L) > 0 ? 1 : 0;
}

// the pointers of a KKT solve (bwd: it has a backward pass, which reads the cost blocks)
static int check_kkt_ptrs(const noc::KKTArgs& a, bool bwd) {
  return check_ptrs({{a.A, "A", true}, {a.Bm, "B", true}, {a.Q, "Q", bwd}, {a.R, "R", bwd},
                     {a.M, "M", bwd}, {a.r, "r", bwd}, {a.P, "P", bwd}, {a.q, "q", false},
                     {a.c, "c", false}, {a.p, "p", false}, {a.x0, "x0", false}, {a.K, "K", false},
                     {a.d, "d", false}, {a.S, "S", false}, {a.v, "v", false}, {a.dx, "dx", false},
                     {a.du, "du", false}, {a.reg, "reg", false, 8}, {a.pred, "pred", false, 8},
                     {a.feasible, "feasible", false, 4}, {a.active, "active", false, 4}});
}

static const char kNeedGains[] = "K and d are required (workspace) unless noc_kkt_gains_on_chip() is 1";

// a: N, B, mode, tiled and the pointers (KKTArgs order; the launcher sets the rest)
static int kkt_run(int nx, int nu, int lanes, const noc::KKTArgs& a, void* stream) {
  int rc = check_dims(nx, nu, a.N, a.B, lanes);
  if (!rc) rc = check_kkt_ptrs(a, a.mode != noc::MODE_FWD);
  if (rc || a.B == 0) return rc;
  if (a.tiled && lanes == 0) return fail(-1, "the tiled layout needs an explicit lanes value");
  if (a.tiled && lanes == 1 && !(nx == 8 && nu == 4))
    return fail(-1, "the grouped (lanes = 1) tiled layout is supported for (nx, nu) = (8, 4)");
  if (lanes == 1 && !(64 % nx == 0 && nu <= nx))
    return fail(-1, "the group solve (lanes = 1) needs nx dividing 64 and nu <= nx");
  const int L = lanes ? lanes : noc::kkt_default_lanes(nx, nu, a.N);
  const bool on_chip = a.mode == noc::MODE_FULL && (a.dx || a.du) && noc::kkt_lds_bytes_rt(nx, nu, a.N, L) > 0;
  if ((!a.K || !a.d) && !on_chip) return fail(-2, kNeedGains);
  return hip_status(noc::kkt_dispatch(nx, nu, a, L, static_cast<hipStream_t>(stream)),
                    "kkt_scan launch");
}

int noc_kkt_solve(int nx, int nu, int N, int B, int lanes, const double* A, const double* Bm,
                  const double* Q, const double* R, const double* M, const double* r,
                  const double* q, const double* c, const double* P, const double* p,
                  const double* x0, const double* reg, const int* active, double* dx, double* du,
                  double* pred, int* feasible, double* K, double* d, double* S, double* v,
                  void* stream) {
  return kkt_run(nx, nu, lanes, {N, B, noc::MODE_FULL, 0, A, Bm, Q, R, M, r, q, c, P, p, x0, reg, active,
                                 dx, du, pred, K, d, S, v, feasible, g_ablate, 0}, stream);
}

int noc_kkt_solve_tiled(int nx, int nu, int N, int B, int lanes, const double* A,
                        const double* Bm, const double* Q, const double* R, const double* M,
                        const double* r, const double* q, const double* c, const double* P,
                        const double* p, const double* x0, const double* reg, const int* active,
                        double* dx, double* du, double* pred, int* feasible, double* K, double* d,
                        double* S, double* v, void* stream) {
  return kkt_run(nx, nu, lanes, {N, B, noc::MODE_FULL, 0, A, Bm, Q, R, M, r, q, c, P, p, x0, reg, active,
                                 dx, du, pred, K, d, S, v, feasible, g_ablate, 1}, stream);
}

int noc_kkt_compact_supported(const noc_family* fam, int N, int lanes) {
  return (fam && N >= 1 && noc::kkt_compact_supported(*fam, lanes)) ? 1 : 0;
}

int noc_compact_width(const noc_family* fam, int field) {
  if (!fam) return fail(-1, "family is NULL");
  const int w = noc::compact_width(*fam, field);
  return w < 0 ? fail(-1, "noc_compact_width: unsupported family or field") : w;
}

int noc_kkt_compact_keep(const noc_family* fam, int lanes) {
  if (!fam) return fail(-1, "family is NULL");
  return noc::kkt_compact_keep(*fam, lanes);
}

// family / dims / lanes of the compact entry points (before any HIP call)
static int check_compact_dims(const noc_family* fam, int N, int B, int lanes) {
  if (!fam) return fail(-1, "family is NULL");
  if (int rc = check_horizon_batch(N, B)) return rc;
  if (!noc::kkt_compact_supported(*fam, lanes))
    return fail(-1, "compact blocks: unsupported family or lanes (" + std::to_string(lanes) +
                        "); pendulum and cart-pole at lanes 8, 16, 32 or 64 (noc_kkt_compact_supported)");
  return 0;
}

// a: the tiled full solve of kkt_run without q, c, p, on compact A, B, Q, R, M
static int kkt_compact_run(const noc_family* fam, int lanes, const noc::KKTArgs& a, void* stream) {
  int rc = check_compact_dims(fam, a.N, a.B, lanes);
  if (!rc) rc = check_kkt_ptrs(a, true);
  if (!rc && a.B > 0) {
    const bool on_chip = (a.dx || a.du) && noc::kkt_lds_bytes_rt(fam->nx, fam->nu, a.N, lanes) > 0;
    rc = (!a.K || !a.d) && !on_chip
             ? fail(-2, kNeedGains)
             : hip_status(noc::kkt_compact_dispatch(*fam, a, lanes, static_cast<hipStream_t>(stream)),
                          "kkt_scan_compact launch");
  }
  return args_as_minus1(rc);
}

int noc_kkt_solve_compact(const noc_family* fam, int N, int B, int lanes, const double* A,
                          const double* Bm, const double* Q, const double* R, const double* M,
                          const double* r, const double* P, const double* x0, const double* reg,
                          const int* active, double* dx, double* du, double* pred, int* feasible,
                          double* K, double* d, double* S, double* v, void* stream) {
  return kkt_compact_run(fam, lanes, {N, B, noc::MODE_FULL, 0, A, Bm, Q, R, M, r, nullptr, nullptr, P,
                                      nullptr, x0, reg, active, dx, du, pred, K, d, S, v, feasible,
                                      g_ablate, 1}, stream);
}

int noc_blocks_expand(const noc_family* fam, int N, int B, int lanes, const double* cA,
                      const double* cB, const double* cQ, const double* cR, const double* cM,
                      double* A, double* Bm, double* Q, double* R, double* M, void* stream) {
  if (check_compact_dims(fam, N, B, lanes) ||
      check_all({cA, cB, cQ, cR, cM, A, Bm, Q, R, M}, "blocks_expand argument", 16))
    return -1;
  if (B == 0) return 0;
  const noc::ExpandArgs e{N, B, lanes, cA, cB, cQ, cR, cM, A, Bm, Q, R, M};
  return hip_status(noc::blocks_expand(*fam, e, static_cast<hipStream_t>(stream)), "blocks_expand");
}

long long noc_tiled_doubles(int N, int B, int lanes, int E) {
  if (N < 1 || B < 0 || lanes < 1 || E < 1) return -1;
  if (lanes == 1)  // grouped layout: whole records of GROUP_T trajectories
    return (long long)((B + noc::GROUP_T - 1) / noc::GROUP_T) * noc::GROUP_T * N * E;
  const long long cmax = (N + lanes - 1) / lanes;
  return (long long)B * cmax * E * lanes;
}

int noc_relayout(int direction, int E, int sym_n, int N, int B, int lanes, const double* src,
                 double* dst, void* stream) {
  if (direction != 0 && direction != 1) return fail(-1, "direction must be 0 or 1");
  if (N < 1 || B < 0 || E < 1) return fail(-1, "bad dims");
  if (!lanes_in(lanes, {1, 8, 16, 32, 64, 128})) return fail(-1, "lanes must be 1/8/16/32/64/128");
  if (sym_n > 0 && E != sym_n * (sym_n + 1) / 2) return fail(-1, "E must be sym_n(sym_n+1)/2");
  if (!src || !dst) return fail(-2, "NULL pointer");
  return hip_status(noc::relayout(direction, E, sym_n, N, B, lanes, src, dst,
                                  static_cast<hipStream_t>(stream)), "relayout");
}

int noc_par_bwd_pass(int nx, int nu, int N, int B, int lanes, const double* A, const double* Bm,
                     const double* Q, const double* R, const double* M, const double* r,
                     const double* q, const double* c, const double* P, const double* p,
                     const double* reg, const int* active, double* K, double* d, double* S,
                     double* v, double* pred, int* feasible, void* stream) {
  return kkt_run(nx, nu, lanes, {N, B, noc::MODE_BWD, 0, A, Bm, Q, R, M, r, q, c, P, p, nullptr, reg,
                                 active, nullptr, nullptr, pred, K, d, S, v, feasible, g_ablate, 0}, stream);
}

int noc_par_fwd_pass(int nx, int nu, int N, int B, int lanes, const double* A, const double* Bm,
                     const double* c, const double* x0, const double* K, const double* d,
                     const int* active, double* du, double* dx, void* stream) {
  return kkt_run(nx, nu, lanes, {N, B, noc::MODE_FWD, 0, A, Bm, nullptr, nullptr, nullptr, nullptr, nullptr,
                                 c, nullptr, nullptr, x0, nullptr, active, dx, du, nullptr,
                                 const_cast<double*>(K), const_cast<double*>(d), nullptr, nullptr, nullptr,
                                 g_ablate, 0}, stream);
}

int noc_family_supported(const noc_family* fam) {
  return (fam && noc::family_supported(*fam)) ? 1 : 0;
}

// fam: NULL where the entry point takes none
static int check_ipm(const noc_family* fam, const noc_ipm_ws* ws) {
  if (!ws) return fail(-2, "workspace is NULL");
  if (ws->Bt < 0 || ws->N < 1) return fail(-1, "workspace dims: need Bt >= 0, N >= 1");
  if (!lanes_in(ws->lanes, {1, 8, 16, 32, 64}))
    return fail(-1, "workspace lanes must be 1, 8, 16, 32 or 64");
  if (ws->lanes == 1 && fam && !(fam->nx == 8 && fam->nu == 4))
    return fail(-1, "workspace lanes = 1 (grouped layout) is supported for nx = 8, nu = 4");
  if (fam && !noc::family_supported(*fam))
    return fail(-1, "unsupported problem family (kind/nx/nu)");
  const void* req[] = {ws->x, ws->u, ws->x0, ws->A, ws->B, ws->Q, ws->R, ws->M, ws->r, ws->P,
                       ws->cx, ws->cu, ws->lc, ws->lam, ws->dx, ws->du, ws->pred, ws->K, ws->d,
                       ws->feasible, ws->phase, ws->kkt_active, ws->it, ws->inner, ws->total_it,
                       ws->kkt_solves, ws->bp, ws->rp, ws->rinc, ws->cost, ws->hu, ws->gnorm,
                       ws->reg};
  for (const void* p : req)
    if (!p) return fail(-2, "a required workspace pointer is NULL");
  return check_ws_flags(ws->flags, "workspace");
}

// ... of the entry points that take a family: it comes first
static int check_fam_ipm(const noc_family* fam, const noc_ipm_ws* ws) {
  if (!fam) return fail(-2, "family is NULL");
  return check_ipm(fam, ws);
}

int noc_ipm_init(const noc_ipm_ws* ws, double bp0, void* stream) {
  int rc = check_ipm(nullptr, ws);
  if (rc || ws->Bt == 0) return rc;
  return hip_status(noc::ipm_init(*ws, bp0, static_cast<hipStream_t>(stream)), "ipm_init");
}

// the compact twins' extra check: the workspace's block fields can be compact for (family, lanes)
static int check_compact(const noc_family* fam, const noc_ipm_ws* ws) {
  if (!noc::kkt_compact_supported(*fam, ws->lanes))
    return fail(-1, "compact blocks: unsupported family or workspace lanes (noc_kkt_compact_supported)");
  return 0;
}

// the _compact twins' first check
static int check_both(const char* who, const noc_family* fam, const noc_ipm_ws* ws) {
  return fam && ws ? 0 : fail(-1, std::string(who) + ": family or workspace is NULL");
}

// Below, one implementation per operation: `compact` = the workspace's blocks are the compact
// fields, `params` = NULL or the per-trajectory records (never both).  The exported dense,
// _compact and _params forms add their own first checks and code mapping.
static int ipm_checks(const noc_family* fam, const noc_ipm_ws* ws, int mode, const int* terminal,
                      bool compact) {
  int rc = check_fam_ipm(fam, ws);
  if (!rc && compact) rc = check_compact(fam, ws);
  if (!rc) rc = check_mode(mode);
  if (!rc && terminal) rc = check_terminal(*terminal);
  return rc;
}

static int ipm_prepare_any(const noc_family* fam, const noc_ipm_ws* ws, int mode, int terminal,
                           bool compact, const double* params, void* stream) {
  int rc = ipm_checks(fam, ws, mode, &terminal, compact);
  if (rc || ws->Bt == 0) return rc;
  return hip_status(noc::ipm_prepare(*fam, *ws, mode, terminal, compact, params,
                                     static_cast<hipStream_t>(stream)), "ipm_prepare");
}

static int ipm_trial_any(const noc_family* fam, const noc_ipm_ws* ws, int mode, const double* params,
                         void* stream) {
  int rc = ipm_checks(fam, ws, mode, nullptr, false);
  if (rc || ws->Bt == 0) return rc;
  return hip_status(noc::ipm_trial(*fam, *ws, mode, params, static_cast<hipStream_t>(stream)),
                    "ipm_trial");
}

// The KKT step of a workspace (active = phase SOLVE), then the trial.  The trial needs dx, du
// only: the gains stay on chip when they fit (ws->K, ws->d otherwise).  The scan reads no cost
// parameter (the blocks carry them); the trial does.
static int kkt_and_trial(const noc_family* fam, const noc_ipm_ws* ws, int mode, bool compact,
                         const double* params, void* stream) {
  const bool on_chip = noc_kkt_gains_on_chip(fam->nx, fam->nu, ws->N, ws->lanes) == 1;
  const noc::KKTArgs a{ws->N, ws->Bt, noc::MODE_FULL, 0, ws->A, ws->B, ws->Q, ws->R, ws->M, ws->r, nullptr,
                       nullptr, ws->P, nullptr, nullptr, ws->reg, ws->kkt_active, ws->dx, ws->du, ws->pred,
                       on_chip ? nullptr : ws->K, on_chip ? nullptr : ws->d, nullptr, nullptr,
                       ws->feasible, g_ablate, 1};
  int rc = compact ? kkt_compact_run(fam, ws->lanes, a, stream)
                   : kkt_run(fam->nx, fam->nu, ws->lanes, a, stream);
  if (rc) return rc;
  return ipm_trial_any(fam, ws, mode, params, stream);
}

// lanes of the step forms: 0 = the workspace's; any other value must equal it (the blocks are
// laid out for it)
static int check_step_lanes(const char* who, const noc_ipm_ws* ws, int lanes) {
  if (ws && lanes != 0 && lanes != ws->lanes)
    return fail(-1, std::string(who) + ": lanes (" + std::to_string(lanes) + ") differs from the workspace's (" +
                        std::to_string(ws->lanes) + "); pass 0 or ws->lanes");
  return 0;
}

static int ipm_step_any(const noc_family* fam, const noc_ipm_ws* ws, int mode, int terminal,
                        bool compact, const double* params, void* stream) {
  int rc = ipm_prepare_any(fam, ws, mode, terminal, compact, params, stream);
  if (rc) return rc;
  return kkt_and_trial(fam, ws, mode, compact, params, stream);
}

static int ipm_step_main_any(const noc_family* fam, const noc_ipm_ws* ws, int mode, int terminal,
                             bool compact, void* stream) {
  int rc = ipm_checks(fam, ws, mode, &terminal, compact);
  if (rc || ws->Bt == 0) return rc;
  rc = hip_status(noc::ipm_prepare_main(*fam, *ws, mode, terminal, compact,
                                        static_cast<hipStream_t>(stream)), "ipm_prepare_main");
  if (rc) return rc;
  return kkt_and_trial(fam, ws, mode, compact, nullptr, stream);
}

int noc_ipm_prepare(const noc_family* fam, const noc_ipm_ws* ws, int mode, int terminal,
                    void* stream) {
  return ipm_prepare_any(fam, ws, mode, terminal, false, nullptr, stream);
}

int noc_ipm_prepare_compact(const noc_family* fam, const noc_ipm_ws* ws, int mode, int terminal,
                            void* stream) {
  if (int rc = check_both("noc_ipm_prepare_compact", fam, ws)) return rc;
  return ipm_prepare_any(fam, ws, mode, terminal, true, nullptr, stream);
}

int noc_ipm_trial(const noc_family* fam, const noc_ipm_ws* ws, int mode, void* stream) {
  return ipm_trial_any(fam, ws, mode, nullptr, stream);
}

int noc_ipm_step(const noc_family* fam, const noc_ipm_ws* ws, int mode, int terminal, int lanes,
                 void* stream) {
  if (int rc = check_step_lanes("noc_ipm_step", ws, lanes)) return rc;
  return ipm_step_any(fam, ws, mode, terminal, false, nullptr, stream);
}

int noc_ipm_step_compact(const noc_family* fam, const noc_ipm_ws* ws, int mode, int terminal,
                         int lanes, void* stream) {
  int rc = check_both("noc_ipm_step_compact", fam, ws);
  if (!rc) rc = check_step_lanes("noc_ipm_step", ws, lanes);
  if (rc) return rc;
  return ipm_step_any(fam, ws, mode, terminal, true, nullptr, stream);
}

int noc_ipm_rollout(const noc_family* fam, const noc_ipm_ws* ws, void* stream) {
  int rc = check_fam_ipm(fam, ws);
  if (rc || ws->Bt == 0) return rc;
  return hip_status(noc::ipm_rollout(*fam, *ws, static_cast<hipStream_t>(stream)), "ipm_rollout");
}

int noc_ipm_promote(const noc_ipm_ws* ws, void* stream) {
  int rc = check_ipm(nullptr, ws);
  if (rc || ws->Bt == 0) return rc;
  return hip_status(noc::ipm_promote(*ws, static_cast<hipStream_t>(stream)), "ipm_promote");
}

int noc_ipm_step_main(const noc_family* fam, const noc_ipm_ws* ws, int mode, int terminal,
                      void* stream) {
  return ipm_step_main_any(fam, ws, mode, terminal, false, stream);
}

int noc_ipm_step_main_compact(const noc_family* fam, const noc_ipm_ws* ws, int mode, int terminal,
                              void* stream) {
  if (int rc = check_both("noc_ipm_step_main_compact", fam, ws)) return rc;
  return ipm_step_main_any(fam, ws, mode, terminal, true, stream);
}

int noc_debug_phase_cycles(long long* out, int n, int reset) {
  if (!out || n < 0) return fail(-2, "out is NULL");
  return noc::debug_phase_cycles(out, n, reset) == 0 ? 0 : fail(-10, "hipMemcpyFromSymbol failed");
}

// Diagnostic export (not in include/noc_hip.h; tools/flip_probe.py): the decision-trace buffer of
// the persistent solvers, (ntraj, cap, 12) doubles; NULL switches it off.  Returns 1 if this build
// records (make trace-lib), 0 if it has no trace code.
extern "C" int noc_debug_set_decision_trace(double* buf, int cap, int ntraj) {
  if (cap < 0 || ntraj < 0) return fail(-1, "cap, ntraj must be >= 0");
  const int rc = noc::debug_set_decision_trace(buf, cap, ntraj);
  return rc < 0 ? fail(-10, "hipMemcpyToSymbol failed") : rc;
}

int noc_debug_traj_times(long long* out, int n) {
  if (!out || n < 0) return fail(-2, "out is NULL");
  return noc::debug_traj_times(out, n) == 0 ? 0 : fail(-10, "hipMemcpyFromSymbol failed");
}

int noc_ipm_solve_supported(const noc_family* fam, int N, int lanes) {
  return (fam && N >= 1 && noc::ipm_solve_supported(*fam, N, lanes)) ? 1 : 0;
}

static int ipm_solve_any(const noc_family* fam, const noc_ipm_ws* ws, int mode, int terminal,
                         double bp0, int max_solves, const double* params, void* stream) {
  int rc = ipm_checks(fam, ws, mode, &terminal, false);
  if (rc) return rc;
  if (!(bp0 > 0.0)) return fail(-1, "bp0 must be > 0");
  if (max_solves < 1) return fail(-1, "max_solves must be >= 1");
  if (!noc::ipm_solve_supported(*fam, ws->N, ws->lanes))
    return fail(-1, "persistent solve needs workspace lanes = 64 and a step that fits in LDS "
                    "(noc_ipm_solve_supported)");
  if (ws->Bt == 0) return 0;
  return hip_status(noc::ipm_solve(*fam, *ws, mode, terminal, bp0, max_solves, params,
                                   static_cast<hipStream_t>(stream)), "ipm_solve");
}

int noc_ipm_solve(const noc_family* fam, const noc_ipm_ws* ws, int mode, int terminal, double bp0,
                  int max_solves, void* stream) {
  return ipm_solve_any(fam, ws, mode, terminal, bp0, max_solves, nullptr, stream);
}

int noc_debug_ipm_plan(const noc_family* fam, int N, int Bt, int flags, int ordered, int with_params,
                       int simds, int* out, int n) {
  if (!fam || !out) return fail(-2, "noc_debug_ipm_plan: family or out is NULL");
  if (n < NOC_PLAN_INTS) return fail(-1, "noc_debug_ipm_plan: out needs NOC_PLAN_INTS entries");
  if (N < 1 || Bt < 0 || simds < 0) return fail(-1, "noc_debug_ipm_plan: need N >= 1, Bt >= 0, simds >= 0");
  if (int rc = check_ws_flags(flags, "noc_debug_ipm_plan:")) return rc;
  noc::debug_ipm_plan(*fam, N, Bt, flags, ordered != 0, with_params != 0, simds, out);
  return 0;
}

long long noc_ddp_work_doubles(int nx, int nu, int N, int Bt) {
  if (nx < 1 || nu < 1 || N < 1 || Bt < 0) return -1;
  const long long b = Bt, n = N;
  // X, TX, TU, k, K and the per-stage derivative records
  return b * (2 * (n + 1) * nx + 2 * n * nu + n * nu * nx + n * noc::ddp_record_doubles(nx, nu));
}

int noc_ddp_supported(const noc_family* fam) { return (fam && noc::ddp_supported(*fam)) ? 1 : 0; }

static int ddp_solve_any(const noc_family* fam, int N, int Bt, const double* x0, double* u,
                         double* work, int* iterations, int* passes, int* done, double bp0,
                         int max_passes, int flags, const double* params, void* stream) {
  if (flags & ~NOC_DDP_ONE_STAGE) return fail(-1, "ddp flags: only NOC_DDP_ONE_STAGE is defined");
  if (!fam) return fail(-2, "family is NULL");
  if (!noc::ddp_supported(*fam))
    return fail(-1, "DDP supports the registered families with nx <= 4 (noc_ddp_supported)");
  if (int rc = check_horizon_batch(N, Bt)) return rc;
  // any finite bp0 >= 0, like the reference ddp (D:98, no check on bp): bp0 = 0 is the
  // unconstrained one-stage solve; the schedule (no NOC_DDP_ONE_STAGE) runs no stage for
  // bp0 <= 1e-4, as interior_point_ddp's while loop (D:194) -- the same rule as the nx > 4 host loop
  if (!(bp0 >= 0.0) || !(bp0 < INFINITY)) return fail(-1, "bp0 must be finite and >= 0");
  if (max_passes < 1) return fail(-1, "max_passes must be >= 1");
  int rc = check_ptrs({{x0, "x0", true, 8}, {u, "u", true, 8}, {work, "work", true, 8},
                       {iterations, "iterations", true, 4}, {passes, "passes", true, 4},
                       {done, "done", true, 4}});
  if (rc || Bt == 0) return rc;
  return hip_status(noc::ddp_solve(*fam, N, Bt, x0, u, work, iterations, passes, done, bp0,
                                   max_passes, flags, params, static_cast<hipStream_t>(stream)),
                    "ddp_solve");
}

int noc_ddp_solve(const noc_family* fam, int N, int Bt, const double* x0, double* u, double* work,
                  int* iterations, int* passes, int* done, double bp0, int max_passes,
                  void* stream) {
  return ddp_solve_any(fam, N, Bt, x0, u, work, iterations, passes, done, bp0, max_passes, 0,
                       nullptr, stream);
}

int noc_ddp_solve_ex(const noc_family* fam, int N, int Bt, const double* x0, double* u,
                     double* work, int* iterations, int* passes, int* done, double bp0,
                     int max_passes, int flags, void* stream) {
  return ddp_solve_any(fam, N, Bt, x0, u, work, iterations, passes, done, bp0, max_passes, flags,
                       nullptr, stream);
}

int noc_ddp_bwd_pass(int nx, int nu, int N, int B, const double* Vx, const double* Vxx,
                     const double* reg_param, const double* cx, const double* cu,
                     const double* cxx, const double* cuu, const double* cxu, const double* fx,
                     const double* fu, const double* fxx, const double* fuu, const double* fxu,
                     double* k, double* K, double* pred, int* feasible, double* Hu, void* stream) {
  if (!noc::kkt_supported(nx, nu))
    return fail(-1, "noc_ddp_bwd_pass: unsupported (nx, nu); supported: " + noc::kkt_shapes_str());
  int rc = check_block_dims(N, B);
  if (!rc) rc = check_all({Vx, Vxx, reg_param, cx, cu, cxx, cuu, cxu, fx, fu, fxx, fuu, fxu, k, K, pred, Hu},
                          "ddp_bwd_pass argument", 8);
  if (!rc) rc = check_ptrs({{feasible, "feasible", true, 4}});
  if (rc || B == 0) return rc;
  noc::DdpBwdArgs a{N, B, Vx, Vxx, reg_param, cx, cu, cxx, cuu, cxu, fx, fu, fxx, fuu, fxu,
                    k, K, pred, Hu, feasible};
  return hip_status(noc::ddp_bwd_pass(nx, nu, a, static_cast<hipStream_t>(stream)), "ddp_bwd_pass");
}

int noc_nonlin_rollout(const noc_family* fam, int N, int B, const double* K, const double* k,
                       const double* x, const double* u, double* x_new, double* u_new,
                       void* stream) {
  int rc = check_family(fam);
  if (!rc) rc = check_block_dims(N, B);
  if (!rc) rc = check_all({K, k, x, u, x_new, u_new}, "nonlin_rollout argument", 8);
  if (rc || B == 0) return rc;
  return hip_status(noc::nonlin_rollout(*fam, N, B, K, k, x, u, x_new, u_new,
                                        static_cast<hipStream_t>(stream)), "nonlin_rollout");
}

// The building blocks that read a cost parameter, each with its _params twin further down.
static int derivatives_any(const noc_family* fam, const noc::DerivArgs& a, const double* params,
                           void* stream) {
  int rc = check_family(fam);
  if (!rc) rc = check_block_dims(a.N, a.B);
  if (!rc) rc = check_all({a.x, a.u, a.bp, a.cx, a.cu, a.cxx, a.cuu, a.cxu, a.fx, a.fu, a.fxx, a.fuu, a.fxu},
                          "derivatives argument", 8);
  if (rc || a.B == 0) return rc;
  return hip_status(noc::derivatives(*fam, a, params, static_cast<hipStream_t>(stream)), "derivatives");
}

static int final_cost_derivs_any(const noc_family* fam, int B, const double* xN, double* grad,
                                 double* hess, const double* params, void* stream) {
  int rc = check_family(fam);
  if (!rc) rc = check_block_dims(1, B);
  if (!rc) rc = check_ptrs({{xN, "xN", true, 8}, {grad, "grad", true, 8}, {hess, "hess", false, 8}});
  if (rc || B == 0) return rc;
  return hip_status(noc::final_cost_derivs(*fam, B, xN, grad, hess, params,
                                           static_cast<hipStream_t>(stream)), "final_cost_derivs");
}

static int check_feasibility_any(const noc_family* fam, int N, int B, const double* x, const double* u,
                                 int* feasible, const double* params, void* stream) {
  int rc = check_family(fam);
  if (!rc) rc = check_block_dims(N, B);
  if (!rc) rc = check_ptrs({{x, "x", true, 8}, {u, "u", true, 8}, {feasible, "feasible", true, 4}});
  if (rc || B == 0) return rc;
  return hip_status(noc::traj_feasibility(*fam, N, B, x, u, feasible, params,
                                          static_cast<hipStream_t>(stream)), "check_feasibility");
}

static int total_cost_any(const noc_family* fam, int N, int B, const double* x, const double* u,
                          const double* bp, double* cost, const double* params, void* stream) {
  int rc = check_family(fam);
  if (!rc) rc = check_block_dims(N, B);
  if (!rc) rc = check_ptrs({{x, "x", true, 8}, {u, "u", true, 8}, {bp, "bp", true, 8}, {cost, "cost", true, 8}});
  if (rc || B == 0) return rc;
  return hip_status(noc::total_cost(*fam, N, B, x, u, bp, cost, params, static_cast<hipStream_t>(stream)),
                    "total_cost");
}

int noc_derivatives(const noc_family* fam, int N, int B, const double* x, const double* u,
                    const double* bp, double* cx, double* cu, double* cxx, double* cuu,
                    double* cxu, double* fx, double* fu, double* fxx, double* fuu, double* fxu,
                    void* stream) {
  return derivatives_any(fam, {N, B, x, u, bp, cx, cu, cxx, cuu, cxu, fx, fu, fxx, fuu, fxu}, nullptr,
                         stream);
}

int noc_final_cost_derivs(const noc_family* fam, int B, const double* xN, double* grad,
                          double* hess, void* stream) {
  return final_cost_derivs_any(fam, B, xN, grad, hess, nullptr, stream);
}

int noc_check_feasibility(const noc_family* fam, int N, int B, const double* x, const double* u,
                          int* feasible, void* stream) {
  return check_feasibility_any(fam, N, B, x, u, feasible, nullptr, stream);
}

int noc_total_cost(const noc_family* fam, int N, int B, const double* x, const double* u,
                   const double* bp, double* cost, void* stream) {
  return total_cost_any(fam, N, B, x, u, bp, cost, nullptr, stream);
}

int noc_costates(int nx, int N, int B, const double* lamT, const double* cx, const double* fx,
                 double* lam, int sequential, void* stream) {
  if (nx < 1 || nx > 8) return fail(-1, "costates support 1 <= nx <= 8");
  int rc = check_block_dims(N, B);
  if (!rc) rc = check_ptrs({{lamT, "lamT", true, 8}, {cx, "cx", true, 8}, {fx, "fx", true, 8},
                            {lam, "lam", true, 8}});
  if (rc || B == 0) return rc;
  return hip_status(noc::costates(nx, N, B, lamT, cx, fx, lam, sequential,
                                  static_cast<hipStream_t>(stream)), "costates");
}

int noc_lqr_params(int nx, int nu, int N, int B, const double* lam, const double* cu,
                   const double* cxx, const double* cuu, const double* cxu, const double* fu,
                   const double* fxx, const double* fuu, const double* fxu, double* ru, double* Q,
                   double* R, double* M, void* stream) {
  if (nx < 1 || nx > 8 || nu < 1 || nu > 8) return fail(-1, "lqr_params support nx, nu <= 8");
  int rc = check_block_dims(N, B);
  if (!rc) rc = check_all({lam, cu, cxx, cuu, cxu, fu, fxx, fuu, fxu, ru, Q, R, M}, "lqr_params argument", 8);
  if (rc || B == 0) return rc;
  noc::LqrArgs a{nx, nu, N, B, lam, cu, cxx, cuu, cxu, fu, fxx, fuu, fxu, ru, Q, R, M};
  return hip_status(noc::lqr_params(a, static_cast<hipStream_t>(stream)), "lqr_params");
}

// ---- per-trajectory cost parameters (include/noc_hip.h) ----------------------------------------
int noc_traj_params_supported(const noc_family* fam, int N, int lanes) {
  if (!fam || N < 1 || !noc::traj_params_supported(*fam)) return 0;
  if (lanes == 1) return (fam->nx == 8 && fam->nu == 4) ? 1 : 0;  // grouped layout (check_ipm)
  return lanes_in(lanes, {8, 16, 32, 64}) ? 1 : 0;
}

// the params record pointer and the family's parametrised cost (w: "<entry point>: ")
static int check_params_ptr(const std::string& w, const noc_family* fam, const double* params) {
  if (!params) return fail(-1, w + "params is NULL (one record of 32 doubles per trajectory)");
  if (reinterpret_cast<uintptr_t>(params) & 15) return fail(-1, w + "params not 16-byte aligned");
  if (!noc::traj_params_supported(*fam))
    return fail(-1, w + "unsupported family (unknown kind / nx / nu, or a registered family with "
                        "traced costs, which has no goal / weights / bound)");
  return 0;
}

// the argument errors of the noc_ipm_*_params entry points, all -1, before any device call
static int check_params(const char* who, const noc_family* fam, const noc_ipm_ws* ws,
                        const double* params) {
  const std::string w = std::string(who) + ": ";
  if (check_both(who, fam, ws) || check_params_ptr(w, fam, params) ||
      check_ws_flags(ws->flags, w + "workspace"))
    return -1;
  if (!noc_traj_params_supported(fam, ws->N, ws->lanes))
    return fail(-1, w + "wrong lanes (" + std::to_string(ws->lanes) + ") or horizon for this family "
                        "(noc_traj_params_supported)");
  return check_ipm(fam, ws) ? -1 : 0;
}

int noc_ipm_prepare_params(const noc_family* fam, const noc_ipm_ws* ws, const double* params,
                           int mode, int terminal, void* stream) {
  if (check_params("noc_ipm_prepare_params", fam, ws, params)) return -1;
  return args_as_minus1(ipm_prepare_any(fam, ws, mode, terminal, false, params, stream));
}

int noc_ipm_trial_params(const noc_family* fam, const noc_ipm_ws* ws, const double* params,
                         int mode, void* stream) {
  if (check_params("noc_ipm_trial_params", fam, ws, params)) return -1;
  return args_as_minus1(ipm_trial_any(fam, ws, mode, params, stream));
}

// (the KKT step's own codes pass through: -3 for a misaligned workspace field)
int noc_ipm_step_params(const noc_family* fam, const noc_ipm_ws* ws, const double* params,
                        int mode, int terminal, int lanes, void* stream) {
  if (int rc = check_step_lanes("noc_ipm_step_params", ws, lanes)) return rc;
  if (check_params("noc_ipm_step_params", fam, ws, params)) return -1;
  return ipm_step_any(fam, ws, mode, terminal, false, params, stream);
}

int noc_ipm_solve_params(const noc_family* fam, const noc_ipm_ws* ws, const double* params,
                         int mode, int terminal, double bp0, int max_solves, void* stream) {
  if (fam && ws && params && noc::traj_params_supported(*fam) && ws->lanes != 64)
    return fail(-1, "noc_ipm_solve_params: wrong lanes (" + std::to_string(ws->lanes) +
                        "): the persistent solve needs workspace lanes = 64");
  if (check_params("noc_ipm_solve_params", fam, ws, params)) return -1;
  return args_as_minus1(ipm_solve_any(fam, ws, mode, terminal, bp0, max_solves, params, stream));
}

// ---- per-trajectory cost parameters in interior-point DDP and the building blocks -------------
int noc_ddp_params_supported(const noc_family* fam) {
  return (fam && noc::ddp_params_supported(*fam)) ? 1 : 0;
}

// the errors the _params forms add to their twins', all -1, before any device call
static int check_block_params(const char* who, const noc_family* fam, const double* params, bool ddp) {
  const std::string w = std::string(who) + ": ";
  if (!fam) return fail(-1, w + "family is NULL");
  if (check_params_ptr(w, fam, params)) return -1;
  if (ddp && !noc::ddp_params_supported(*fam))
    return fail(-1, w + "unsupported family for the one-launch DDP kernel: nx <= 4 "
                        "(noc_ddp_params_supported)");
  return 0;
}

int noc_ddp_solve_params(const noc_family* fam, int N, int Bt, const double* x0, double* u,
                         double* work, int* iterations, int* passes, int* done,
                         const double* params, double bp0, int max_passes, int flags, void* stream) {
  if (check_block_params("noc_ddp_solve_params", fam, params, true)) return -1;
  return args_as_minus1(ddp_solve_any(fam, N, Bt, x0, u, work, iterations, passes, done, bp0,
                                      max_passes, flags, params, stream));
}

int noc_derivatives_params(const noc_family* fam, int N, int B, const double* x, const double* u,
                           const double* bp, double* cx, double* cu, double* cxx, double* cuu,
                           double* cxu, double* fx, double* fu, double* fxx, double* fuu,
                           double* fxu, const double* params, void* stream) {
  if (check_block_params("noc_derivatives_params", fam, params, false)) return -1;
  return args_as_minus1(derivatives_any(
      fam, {N, B, x, u, bp, cx, cu, cxx, cuu, cxu, fx, fu, fxx, fuu, fxu}, params, stream));
}

int noc_final_cost_derivs_params(const noc_family* fam, int B, const double* xN, double* grad,
                                 double* hess, const double* params, void* stream) {
  if (check_block_params("noc_final_cost_derivs_params", fam, params, false)) return -1;
  return args_as_minus1(final_cost_derivs_any(fam, B, xN, grad, hess, params, stream));
}

int noc_check_feasibility_params(const noc_family* fam, int N, int B, const double* x,
                                 const double* u, int* feasible, const double* params,
                                 void* stream) {
  if (check_block_params("noc_check_feasibility_params", fam, params, false)) return -1;
  return args_as_minus1(check_feasibility_any(fam, N, B, x, u, feasible, params, stream));
}

int noc_total_cost_params(const noc_family* fam, int N, int B, const double* x, const double* u,
                          const double* bp, double* cost, const double* params, void* stream) {
  if (check_block_params("noc_total_cost_params", fam, params, false)) return -1;
  return args_as_minus1(total_cost_any(fam, N, B, x, u, bp, cost, params, stream));
}

}  // extern "C"
