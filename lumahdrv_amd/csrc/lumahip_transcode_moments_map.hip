// lumahip_transcode_moments_map.hip -- the transcode moments map kernels (lh::k_transcode_moments_map, luma_kernels.hpp): the five
// sums of lumahip_moments_map_frames_device per block of 8, 16, 32 or 64 luma pixels squared, e taken from the transcode of source
// planes instead of the encode of float frames, every word of the map written once by one launch.  Named here and nowhere else:
// their own translation unit, so that the 48 kernels compile side by side with the other units and no kernel is in two code
// objects.  What a launch may be (transcode_plan), the dispatch (measure_planes_impl) and the entry point are lumahip_transcode.hip's.
#include "lumahip_internal.hpp"
#include "lumahip_pick.hpp"

namespace lhost {
transdist_map_kernel_t pick_transdist_moments_map(int vw, int csd, bool subd, int cse, bool sube, int mode)
{
    return vw == 4 ? pick_planes<TransMomentsMapFamily, 4>(csd, subd, cse, sube, mode) : pick_planes<TransMomentsMapFamily, 2>(csd, subd, cse, sube, mode);
}
}  // namespace lhost
