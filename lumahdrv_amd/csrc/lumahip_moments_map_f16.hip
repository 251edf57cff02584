// lumahip_moments_map_f16.hip -- the binary16-frame moments map kernels (lh::k_moments_map<..., IN16 = true>, luma_kernels.hpp), named
// here and nowhere else: their own translation unit, so that they compile side by side with the float kernels of
// lumahip_moments_map.hip.
#include "lumahip_internal.hpp"
#include "lumahip_pick.hpp"

namespace lhost {
map_kernel_t pick_moments_map_f16(int cs, bool sub, int vw, int mode) { return pick_dist<MomentsMapFamily, true>(cs, sub, vw, mode); }
}  // namespace lhost
