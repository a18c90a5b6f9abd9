// Host side of the compact (structure-aware) LQ blocks outside the persistent solver: which
// families / lanes the stand-alone compact scan covers, the compact fields' widths, the dispatch
// to the scan's instances (kkt_scan_compact_*.hip) and the kernel that expands compact fields into
// the dense tiled ones (natural_blocks(), the two-wave fallback).  See kkt_compact_src.h.
#include <hip/hip_runtime.h>

#include "../../include/noc_hip.h"
#include "block_struct.h"
#include "noc_internal.h"
#include "small_linalg.h"

namespace noc {

#ifndef NOC_CUSTOM_FAMILY  // a registered family's build has no compact scan (its entries report so)
template <int KIND, int NX, int NU, int L>
hipError_t launch_kkt_compact(const noc_family& prm, const KKTArgs& a, hipStream_t stream);

// the families with a compact scan: X(kind, nx, nu)
#define NOC_COMPACT_FAMILIES(X) X(NOC_FAMILY_CARTPOLE, 4, 1) X(NOC_FAMILY_PENDULUM, 2, 1)

// thread per (trajectory, chunk slot, lane) in tiled order, as linearize_kernel
template <int KIND, int NX, int NU>
__global__ __launch_bounds__(256) void blocks_expand_kernel(noc_family prm, ExpandArgs e) {
  using BS = BlockStruct<KIND, NX, NU, true>;
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int L = e.lanes;
  const Chunks ch(e.N, L);
  if (t >= (long long)e.B * ch.cmax * L) return;
  const int b = (int)(t / ((long long)ch.cmax * L));
  const int rem = (int)(t % ((long long)ch.cmax * L));
  const int j = rem / L, l = rem % L;
  if (j >= ch.len(l)) return;
  auto field = [&](auto F, const double* src, double* dst) {
    constexpr int f = decltype(F)::value;
    constexpr int EV = BS::template nv<f>(), E = BS::template size<f>();
    double v[EV > 0 ? EV : 1], full[E];
    if constexpr (EV > 0) tload_rt<EV>(src, L, ch.cmax, b, j, l, v);
    BS::template expand<f>(prm, v, full);
    tstore_rt<E>(dst, L, ch.cmax, b, j, l, full);
  };
  field(std::integral_constant<int, BF_A>{}, e.cA, e.A);
  field(std::integral_constant<int, BF_B>{}, e.cB, e.Bm);
  field(std::integral_constant<int, BF_Q>{}, e.cQ, e.Q);
  field(std::integral_constant<int, BF_R>{}, e.cR, e.R);
  field(std::integral_constant<int, BF_M>{}, e.cM, e.M);
}

template <int KIND, int NX, int NU>
static int width_t(int field) {
  using BS = BlockStruct<KIND, NX, NU, true>;
  switch (field) {
    case BF_A: return BS::template nv<BF_A>();
    case BF_B: return BS::template nv<BF_B>();
    case BF_Q: return BS::template nv<BF_Q>();
    case BF_R: return BS::template nv<BF_R>();
    case BF_M: return BS::template nv<BF_M>();
    default: return -1;
  }
}

template <int KIND, int NX, int NU>
static hipError_t dispatch_t(const noc_family& p, const KKTArgs& a, int lanes, hipStream_t stream) {
  switch (lanes) {
    case 64: return launch_kkt_compact<KIND, NX, NU, 64>(p, a, stream);
    case 32: return launch_kkt_compact<KIND, NX, NU, 32>(p, a, stream);
    case 16: return launch_kkt_compact<KIND, NX, NU, 16>(p, a, stream);
    case 8: return launch_kkt_compact<KIND, NX, NU, 8>(p, a, stream);
    default: return hipErrorInvalidValue;
  }
}

static bool compact_family(const noc_family& p) {
#define X(K, NX, NU) if (p.kind == K && p.nx == NX && p.nu == NU) return true;
  NOC_COMPACT_FAMILIES(X)
#undef X
  return false;
}

bool kkt_compact_supported(const noc_family& p, int lanes) {
  return compact_family(p) && (lanes == 8 || lanes == 16 || lanes == 32 || lanes == 64);
}

int compact_width(const noc_family& p, int field) {
#define X(K, NX, NU) if (p.kind == K && p.nx == NX && p.nu == NU) return width_t<K, NX, NU>(field);
  NOC_COMPACT_FAMILIES(X)
#undef X
  return -1;
}

int kkt_compact_keep(const noc_family& p, int lanes) {
  return kkt_compact_supported(p, lanes) ? compact_keep(p.kind, lanes) : -1;
}

hipError_t kkt_compact_dispatch(const noc_family& p, const KKTArgs& a, int lanes, hipStream_t stream) {
#define X(K, NX, NU) if (p.kind == K && p.nx == NX && p.nu == NU) return dispatch_t<K, NX, NU>(p, a, lanes, stream);
  NOC_COMPACT_FAMILIES(X)
#undef X
  return hipErrorInvalidValue;
}

hipError_t blocks_expand(const noc_family& p, const ExpandArgs& e, hipStream_t stream) {
  const long long cmax = (e.N + e.lanes - 1) / e.lanes;
  const unsigned grid = (unsigned)(((long long)e.B * cmax * e.lanes + 255) / 256);
#define X(K, NX, NU)                                                                              \
  if (p.kind == K && p.nx == NX && p.nu == NU) {                                                  \
    hipLaunchKernelGGL((blocks_expand_kernel<K, NX, NU>), dim3(grid), dim3(256), 0, stream, p, e); \
    return hipGetLastError();                                                                     \
  }
  NOC_COMPACT_FAMILIES(X)
#undef X
  return hipErrorInvalidValue;
}

#else  // NOC_CUSTOM_FAMILY

bool kkt_compact_supported(const noc_family&, int) { return false; }
int compact_width(const noc_family&, int) { return -1; }
int kkt_compact_keep(const noc_family&, int) { return -1; }
hipError_t kkt_compact_dispatch(const noc_family&, const KKTArgs&, int, hipStream_t) { return hipErrorInvalidValue; }
hipError_t blocks_expand(const noc_family&, const ExpandArgs&, hipStream_t) { return hipErrorInvalidValue; }

#endif

}  // namespace noc
