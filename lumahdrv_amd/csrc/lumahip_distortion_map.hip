// lumahip_distortion_map.hip -- the float-frame distortion map kernels (lh::k_distortion_map, luma_kernels.hpp): what
// lumahip_distortion_frames_device sums per frame, per block of 16, 32 or 64 luma pixels squared, every word of the map written once
// by one launch.  Named here and nowhere else: their own translation unit (lumahip_distortion_map_f16.hip holds the binary16-frame
// kernels), so that they compile side by side with the other units' and no kernel is in two code objects.  The dispatch
// (measure_frames_impl) and the entry points are lumahip_distortion.hip's.
#include "lumahip_internal.hpp"
#include "lumahip_pick.hpp"

namespace lhost {
map_kernel_t pick_dist_map_f32(int cs, bool sub, int vw, int mode) { return pick_dist<DistMapFamily, false>(cs, sub, vw, mode); }
}  // namespace lhost
