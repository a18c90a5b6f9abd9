// Instantiation unit of the compact KKT scan (kkt_compact_src.h): cart-pole (4, 1), lanes 32.
#include "kkt_compact_src.h"

namespace noc {
template hipError_t launch_kkt_compact<NOC_FAMILY_CARTPOLE, 4, 1, 32>(const noc_family&, const KKTArgs&, hipStream_t);
}  // namespace noc
