// lumahip_transcode_half_distortion_map.hip -- the half-resolution transcode distortion map kernels
// (lh::k_transcode_half_distortion_map, luma_kernels.hpp): what lumahip_transcode_half_distortion_frames_device sums per frame, per block
// of 16, 32 or 64 luma pixels squared of the half-size target, every word of the map written once by one launch.  Named here and
// nowhere else: their own translation unit, so that the kernels compile side by side with the other units and no kernel is in two code
// objects.  What a launch may be (transcode_plan, scale 2), the dispatch (measure_planes_impl) and the entry point are
// lumahip_transcode.hip's.
#include "lumahip_internal.hpp"
#include "lumahip_pick.hpp"

namespace lhost {
transdist_map_kernel_t pick_transhalf_dist_map(int vw, int csd, bool subd, int cse, bool sube, int mode)
{
    return vw == 4 ? pick_planes<TransHalfDistMapFamily, 4>(csd, subd, cse, sube, mode)
                   : pick_planes<TransHalfDistMapFamily, 2>(csd, subd, cse, sube, mode);
}
}  // namespace lhost
