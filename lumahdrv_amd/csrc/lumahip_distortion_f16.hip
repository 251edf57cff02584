// lumahip_distortion_f16.hip -- the binary16-frame distortion kernels (lh::k_distortion<..., IN16 = true>, luma_kernels.hpp), named
// here and nowhere else: their own translation unit, so that they compile side by side with the float kernels of
// lumahip_distortion.hip, which holds the dispatch (measure_frames_impl) and the entry points.
#include "lumahip_internal.hpp"
#include "lumahip_pick.hpp"

namespace lhost {
dist_kernel_t pick_dist_f16(int cs, bool sub, int vw, int mode) { return pick_dist<DistFamily, true>(cs, sub, vw, mode); }
}  // namespace lhost
