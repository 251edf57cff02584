// lumahip_transcode_distortion.hip -- the transcode distortion kernels (lh::k_transcode_distortion, luma_kernels.hpp): how far given
// code planes are from the planes lumahip_transcode_frames_device would write for the same source planes, as integer sums per frame
// and plane.  Named here and nowhere else: their own translation unit, so that the 48 kernels compile side by side with the other
// units and no kernel is in two code objects.  What a launch may be (transcode_plan), the dispatch (measure_planes_impl) and the
// entry point are lumahip_transcode.hip's.
#include "lumahip_internal.hpp"
#include "lumahip_pick.hpp"

namespace lhost {
transdist_kernel_t pick_transdist(int vw, int csd, bool subd, int cse, bool sube, int mode)
{
    return vw == 4 ? pick_planes<TransDistFamily, 4>(csd, subd, cse, sube, mode) : pick_planes<TransDistFamily, 2>(csd, subd, cse, sube, mode);
}
}  // namespace lhost
