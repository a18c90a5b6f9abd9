// Structure-aware ("compact") block source of the KKT scan, and the stand-alone scan on it.
//
// The compact tiled fields hold only the variable entries of a stage's A, B, Q, R, M
// (block_struct.h: the tiled layout of include/noc_hip.h with E = the field's variable count);
// CompactSrc rebuilds the constant entries where the scan reads a stage -- the doubles the dense
// blocks hold -- and its Struct tells the scan's arithmetic which products have a structural zero.
// Users: the persistent interior-point solver (ipm_persistent.hip) and the stand-alone compact
// scan below (noc_kkt_solve_compact; instantiated in kkt_scan_compact_*.hip), whose results equal
// the dense scan's bit for bit (tests/test_kkt_compact_gpu.py).
#pragma once
#include <hip/hip_runtime.h>

#include "block_struct.h"
#include "kkt_scan_impl.h"

namespace noc {

// BS = BlockStruct<..., false> is the dense layout (the persistent solver's NOC_PERSIST_STRUCT=0
// instance), which loads exactly what ArgsSrc does.
template <class BS, int NX, int NU, int L>
struct CompactSrc {
  using Struct = BS;
  const KKTArgs& a;
  const noc_family& p;
  int traj, l, cmax;
  size_t tN;
  template <int F, bool LAST = false>
  NOC_DEV void field(const double* base, int j, double* full) const {
    constexpr int EV = BS::template nv<F>();
    double v[EV > 0 ? EV : 1];
    if constexpr (EV > 0) tload_pol<EV, L, LAST>(base, traj, j, l, cmax, v);
    BS::template expand<F>(p, v, full);
  }
  // PART / LAST: as load_stage (kkt_scan_impl.h)
  template <int PART, bool LAST = false>
  NOC_DEV void stage_part(int, int j, StageData<NX, NU>& st) const {
    constexpr bool REST = PART != 2, WQ = PART != 1, WAB = REST && PART != 3;
    if constexpr (WAB) {
      field<BF_A>(a.A, j, st.A.v);
      field<BF_B>(a.Bm, j, st.B.v);
    }
    if constexpr (WQ) field<BF_Q, LAST>(a.Q, j, st.Q.v);
    if constexpr (REST) {
      field<BF_R, LAST>(a.R, j, st.R.v);
      field<BF_M, LAST>(a.M, j, st.M.v);
      tload_pol<NU, L, LAST>(a.r, traj, j, l, cmax, st.r.v);
    }
  }
  NOC_DEV void stage(int s, int j, StageData<NX, NU>& st) const { stage_part<0>(s, j, st); }
  NOC_DEV void stage_last(int s, int j, StageData<NX, NU>& st) const { stage_part<0, true>(s, j, st); }
  NOC_DEV void ab(int, int j, Mat<NX, NX>& A, Mat<NX, NU>& Bm, Vec<NX>& c) const {
    field<BF_A, true>(a.A, j, A.v);  // phase 4: the last read of A, B (non-temporal)
    field<BF_B, true>(a.Bm, j, Bm.v);
    set_zero(c);
  }
  NOC_DEV void cvec(int, int, Vec<NX>& c) const { set_zero(c); }
  // The compact A, B record of a stage the scan keeps on chip from phase 3 to phase 4
  // (kkt_scan_wave_src: KEEP): pack_ab takes the variable entries back out of the expanded blocks,
  // unpack_ab is ab() on the record instead of on memory -- the same expand, the same doubles.
  static constexpr int kNvA = BS::template nv<BF_A>(), kNvB = BS::template nv<BF_B>();
  static constexpr int kRecAB = kNvA + kNvB;
  NOC_DEV void pack_ab(const Mat<NX, NX>& A, const Mat<NX, NU>& Bm, double* rec) const {
    BS::template compress<BF_A>(A.v, rec);
    BS::template compress<BF_B>(Bm.v, rec + kNvA);
  }
  NOC_DEV void unpack_ab(const double* rec, Mat<NX, NX>& A, Mat<NX, NU>& Bm, Vec<NX>& c) const {
    BS::template expand<BF_A>(p, rec, A.v);
    BS::template expand<BF_B>(p, rec + kNvA, Bm.v);
    set_zero(c);
  }
};

// kkt_scan_compact_kernel's options, from its template parameters: kkt_scan_kernel's, with the kept
// slots, without the A, B slots in LDS and the non-temporal phase 3 (the compact blocks of the
// batches those exist for stay within the memory-side cache)
template <int CACHE_, bool BIG_, int KEEP_>
struct CompactKernelOpt : ScanOpt {
  static constexpr int CACHE = CACHE_, KEEP = KEEP_;
  static constexpr bool BIG = BIG_, AB = false, PEEL = true, FOLD = true;
};

// The stand-alone scan on compact blocks: kkt_scan_kernel's tiled, non-affine instance with the
// blocks read through CompactSrc (a.A, a.Bm, a.Q, a.R, a.M: the compact fields).  Same dead-wave /
// barrier prologue, same register budgets (BIG: one wave per SIMD).
template <int KIND, int NX, int NU, int L, int CACHE, bool BIG, int KEEP = 0>
__global__ __launch_bounds__(256, BIG ? 1 : NOC_KKT_WAVES_PER_SIMD) void kkt_scan_compact_kernel(noc_family prm,
                                                                                             KKTArgs a) {
  static_assert(L <= 64, "one-wave segments");
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  if constexpr (BIG) asm volatile("" ::: "a255");  // the whole register file, as kkt_scan_kernel
  const int traj = tid / L;
  if (!scan_lane_live(a, traj)) return;
  using BS = BlockStruct<KIND, NX, NU, true>;
  const int l = tid % L;
  const int cmax = a.N / L + (a.N % L ? 1 : 0);
  const CompactSrc<BS, NX, NU, L> src{a, prm, traj, l, cmax, (size_t)traj * a.N};
  kkt_scan_wave_src<NX, NU, L, false, true, CompactSrc<BS, NX, NU, L>, CompactKernelOpt<CACHE, BIG, KEEP>>(a, traj, l,
                                                                                                            src);
}

// launch_kkt's geometry (kkt_launch_geometry) for the compact kernel; the A, B slots stay off.
// Instantiated per (family, lanes) in kkt_scan_compact_*.hip.
template <int KIND, int NX, int NU, int L>
hipError_t launch_kkt_compact(const noc_family& prm, const KKTArgs& a_in, hipStream_t stream) {
  static_assert(L <= 64, "one-wave segments");
  KKTArgs a = a_in;
  constexpr int CC = kkt_cache_len<NX, NU, L>();
  constexpr bool kHasBig = (L == 64 || L == 32) && NX >= 3 && NX <= 4;  // (kkt_launch_geometry: big)
  constexpr int KP = compact_keep(KIND, L);  // the streamed instances' kept slots (block_struct.h)
  const auto [cached, big, lds, block, grid, ok] = kkt_launch_geometry<NX, NU, L, false>(a);
  a.tiled = 1;
  if (!ok) return hipErrorInvalidValue;  // K/d needed as workspace
  if (cached) {
    if constexpr (CC > 0)
      hipLaunchKernelGGL((kkt_scan_compact_kernel<KIND, NX, NU, L, CC, false>), dim3(grid), dim3(block), lds, stream,
                         prm, a);
  } else if (big) {
    if constexpr (kHasBig)
      hipLaunchKernelGGL((kkt_scan_compact_kernel<KIND, NX, NU, L, 0, true, KP>), dim3(grid), dim3(block), lds, stream,
                         prm, a);
  } else {
    hipLaunchKernelGGL((kkt_scan_compact_kernel<KIND, NX, NU, L, 0, false, KP>), dim3(grid), dim3(block), lds, stream,
                       prm, a);
  }
  return hipGetLastError();
}

}  // namespace noc
