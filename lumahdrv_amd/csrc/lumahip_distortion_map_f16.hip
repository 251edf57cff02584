// lumahip_distortion_map_f16.hip -- the binary16-frame distortion map kernels (lh::k_distortion_map<..., IN16 = true>, luma_kernels.hpp)
// and the C entry points lumahip_distortion_map_frames_device_f16 / _planar_f16.  Their own translation unit so that they compile
// side by side with the float kernels of lumahip_distortion_map.hip.
#include "lumahip_internal.hpp"
#include "lumahip_pick.hpp"

using namespace lh;
using namespace lhost;

namespace lhost {
dist_map_kernel_t pick_dist_map_f16(int cs, bool sub, int vw, int mode) { return pick_dist<DistMapFamily, true>(cs, sub, vw, mode); }
}  // namespace lhost

extern "C" int lumahip_distortion_map_frames_device_f16(lumahip_ctx *c, const uint16_t *rgb, size_t frame_stride, unsigned nframes, unsigned w,
                                                        unsigned h, float sc, int profile, const unsigned char *const planes[3],
                                                        const int stride[3], const size_t pfs[3], unsigned block, uint64_t *map_dev)
{
    if (!c)
        return LUMAHIP_ERR_ARG;
    if (!rgb)
        return fail(c, LUMAHIP_ERR_ARG, "null argument");
    return distortion_map_impl(c, packed_frames(rgb, frame_stride, nframes, w, h), sc, {planes, stride, pfs, profile}, block, map_dev,
                               {c->stream, true});
}

extern "C" int lumahip_distortion_map_frames_device_planar_f16(lumahip_ctx *c, const uint16_t *const rgb_planes[3], size_t frame_stride,
                                                               unsigned nframes, unsigned w, unsigned h, float sc, int profile,
                                                               const unsigned char *const planes[3], const int stride[3], const size_t pfs[3],
                                                               unsigned block, uint64_t *map_dev)
{
    if (!c)
        return LUMAHIP_ERR_ARG;
    return distortion_map_impl(c, planar_frames(rgb_planes, frame_stride, nframes, w, h), sc, {planes, stride, pfs, profile}, block, map_dev,
                               {c->stream, true});
}
