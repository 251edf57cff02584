// lumahip_encode_f16.hip -- the binary16-frame encode kernels (lh::k_encode<..., IN16 = true>, luma_kernels.hpp) and the C entry
// points lumahip_encode_frames_device_f16 / _planar_f16.  Their own translation unit so that they compile side by side with the
// float kernels of lumahip_encode.hip (and with the same scheduling strategy, flags.mk).
#include "lumahip_internal.hpp"
#include "lumahip_pick.hpp"

using namespace lh;
using namespace lhost;

namespace lhost {
enc_kernel_t pick_enc_f16(int cs, bool sub, int vw, int mode) { return pick_enc<true>(cs, sub, vw, mode); }
}  // namespace lhost

extern "C" int lumahip_encode_frames_device_f16(lumahip_ctx *c, const uint16_t *rgb, size_t frame_stride, unsigned nframes,
                                                unsigned w, unsigned h, float sc, int profile, unsigned char *const planes[3],
                                                const int stride[3], const size_t pfs[3], float *stats)
{
    if (!c)
        return LUMAHIP_ERR_ARG;
    if (!rgb)
        return fail(c, LUMAHIP_ERR_ARG, "null argument");
    if (!c->have_quant)
        return fail(c, LUMAHIP_ERR_STATE, "quantizer not set");
    return encode_frames_device_impl(c, packed_frames(rgb, frame_stride, nframes, w, h), sc, {planes, stride, pfs, profile}, stats,
                                     {c->q.cs, c->stream, true, HalfSource::Typed});
}

extern "C" int lumahip_encode_frames_device_planar_f16(lumahip_ctx *c, const uint16_t *const rgb_planes[3], size_t frame_stride,
                                                       unsigned nframes, unsigned w, unsigned h, float sc, int profile,
                                                       unsigned char *const planes[3], const int stride[3], const size_t pfs[3],
                                                       float *stats)
{
    if (!c)
        return LUMAHIP_ERR_ARG;
    if (!rgb_planes)
        return fail(c, LUMAHIP_ERR_ARG, "null argument");
    if (!c->have_quant)
        return fail(c, LUMAHIP_ERR_STATE, "quantizer not set");
    return encode_frames_device_impl(c, planar_frames(rgb_planes, frame_stride, nframes, w, h), sc, {planes, stride, pfs, profile}, stats,
                                     {c->q.cs, c->stream, true, HalfSource::Typed});
}
