// lumahip_transcode_half_distortion.hip -- the half-resolution transcode distortion kernels (lh::k_transcode_half_distortion,
// luma_kernels.hpp): given code planes of (w/2) x (h/2) against what lumahip_transcode_half_frames_device would write for source planes
// of w x h, 12 words per frame, one launch.  Named here and nowhere else: their own translation unit, so that the kernels compile side
// by side with the other units and no kernel is in two code objects.  What a launch may be (transcode_plan, scale 2), the dispatch
// (measure_planes_impl) and the entry point are lumahip_transcode.hip's.
#include "lumahip_internal.hpp"
#include "lumahip_pick.hpp"

namespace lhost {
transdist_kernel_t pick_transhalf_dist(int vw, int csd, bool subd, int cse, bool sube, int mode)
{
    return vw == 4 ? pick_planes<TransHalfDistFamily, 4>(csd, subd, cse, sube, mode) : pick_planes<TransHalfDistFamily, 2>(csd, subd, cse, sube, mode);
}
}  // namespace lhost
