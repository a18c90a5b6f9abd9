// Instantiation unit of the compact KKT scan (kkt_compact_src.h): pendulum (2, 1), lanes 8 - 64.
#include "kkt_compact_src.h"

namespace noc {
template hipError_t launch_kkt_compact<NOC_FAMILY_PENDULUM, 2, 1, 8>(const noc_family&, const KKTArgs&, hipStream_t);
template hipError_t launch_kkt_compact<NOC_FAMILY_PENDULUM, 2, 1, 16>(const noc_family&, const KKTArgs&, hipStream_t);
template hipError_t launch_kkt_compact<NOC_FAMILY_PENDULUM, 2, 1, 32>(const noc_family&, const KKTArgs&, hipStream_t);
template hipError_t launch_kkt_compact<NOC_FAMILY_PENDULUM, 2, 1, 64>(const noc_family&, const KKTArgs&, hipStream_t);
}  // namespace noc
