// lumahip_moments_map.hip -- the float-frame moments map kernels (lh::k_moments_map, luma_kernels.hpp): per block of 8, 16, 32 or 64
// luma pixels squared and per plane the five sums a structural-similarity index needs of the frames' codes e and the given samples g
// -- sum e, sum g, sum e^2, sum g^2, sum e g --, every word of the map written once by one launch.  Named here and nowhere else: their
// own translation unit (lumahip_moments_map_f16.hip holds the binary16-frame kernels), so that they compile side by side with the
// other units' and no kernel is in two code objects.  The dispatch (measure_frames_impl) and the entry points are
// lumahip_distortion.hip's.
#include "lumahip_internal.hpp"
#include "lumahip_pick.hpp"

namespace lhost {
map_kernel_t pick_moments_map_f32(int cs, bool sub, int vw, int mode) { return pick_dist<MomentsMapFamily, false>(cs, sub, vw, mode); }
}  // namespace lhost
