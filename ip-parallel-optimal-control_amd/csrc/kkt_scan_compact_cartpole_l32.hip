// Instantiation unit of the compact KKT scan (kkt_compact_src.h): cart-pole (4, 1), lanes 32.
#include "kkt_compact_src.h"

namespace noc {
template hipError_t launch_kkt_compact<NOC_FAMILY_CARTPOLE, 4, 1, 32>(const noc_family&, const KKTArgs&, hipStream_t);
}  // namespace noc

#ifdef NOC_SCAN_STAMPS
// diagnostic export of the compact stamps build (`make stamps-compact-lib`; not part of the ABI
// header): as kkt_scan_4x1.hip's, for this unit's own stamp table (the c3 launch)
extern "C" int noc_debug_scan_stamps(long long* out, int waves, int reset) {
  if (waves > noc::kStampWaves) waves = noc::kStampWaves;
  const size_t bytes = (size_t)waves * noc::kStampSlots * 2 * sizeof(long long);
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(noc::g_scan_stamps), bytes) != hipSuccess) return -1;
  if (reset) {
    void* p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(noc::g_scan_stamps)) != hipSuccess) return -1;
    if (hipMemset(p, 0, sizeof(noc::g_scan_stamps)) != hipSuccess) return -1;
  }
  return 0;
}
#endif
