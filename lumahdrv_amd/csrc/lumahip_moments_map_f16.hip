// lumahip_moments_map_f16.hip -- the binary16-frame moments map kernels (lh::k_moments_map<..., IN16 = true>, luma_kernels.hpp) and the
// C entry points lumahip_moments_map_frames_device_f16 / _planar_f16.  Their own translation unit so that they compile side by side
// with the float kernels of lumahip_moments_map.hip.
#include "lumahip_internal.hpp"
#include "lumahip_pick.hpp"

using namespace lh;
using namespace lhost;

namespace lhost {
moments_map_kernel_t pick_moments_map_f16(int cs, bool sub, int vw, int mode) { return pick_dist<MomentsMapFamily, true>(cs, sub, vw, mode); }
}  // namespace lhost

extern "C" int lumahip_moments_map_frames_device_f16(lumahip_ctx *c, const uint16_t *rgb, size_t frame_stride, unsigned nframes, unsigned w,
                                                     unsigned h, float sc, int profile, const unsigned char *const planes[3],
                                                     const int stride[3], const size_t pfs[3], unsigned block, uint64_t *mom_dev)
{
    if (!c)
        return LUMAHIP_ERR_ARG;
    if (!rgb)
        return fail(c, LUMAHIP_ERR_ARG, "null argument");
    return moments_map_impl(c, packed_frames(rgb, frame_stride, nframes, w, h), sc, {planes, stride, pfs, profile}, block, mom_dev,
                            {c->stream, true});
}

extern "C" int lumahip_moments_map_frames_device_planar_f16(lumahip_ctx *c, const uint16_t *const rgb_planes[3], size_t frame_stride,
                                                            unsigned nframes, unsigned w, unsigned h, float sc, int profile,
                                                            const unsigned char *const planes[3], const int stride[3], const size_t pfs[3],
                                                            unsigned block, uint64_t *mom_dev)
{
    if (!c)
        return LUMAHIP_ERR_ARG;
    return moments_map_impl(c, planar_frames(rgb_planes, frame_stride, nframes, w, h), sc, {planes, stride, pfs, profile}, block, mom_dev,
                            {c->stream, true});
}
