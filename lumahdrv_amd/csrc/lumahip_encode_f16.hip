// lumahip_encode_f16.hip -- the binary16-frame encode kernels (lh::k_encode<..., IN16 = true>, luma_kernels.hpp) and the C entry
// points lumahip_encode_frames_device_f16 / _planar_f16.  Their own translation unit so that they compile side by side with the
// float kernels of lumahip_encode.hip (and with the same scheduling strategy, flags.mk).
#include "lumahip_internal.hpp"

using namespace lh;
using namespace lhost;

// The same choice as pick_enc2 (lumahip_encode.hip) for frames that are binary16 by type: every search mode, both vector widths,
// and for YCbCr the half-input table kernels (mode 6).  The composite-record kernels without the table (mode 5) are not
// instantiated: frames of halves take the table whenever it exists (encode_frames_device_impl), else the general kernel.
template <int CS, bool SUB>
static enc_kernel_t pick_enc2_f16(int vw, int mode)
{
    if constexpr (CS == CS_YCBCR) {
        if (mode == 6)
            return vw == 4 ? k_encode<CS, SUB, 4, 6, true> : k_encode<CS, SUB, 2, 6, true>;
    }
    if (mode == LUT_THRESH_LDS)
        return vw == 4 ? k_encode<CS, SUB, 4, 3, true> : k_encode<CS, SUB, 2, 3, true>;
    if (mode == LUT_THRESH_GLOBAL)
        return vw == 4 ? k_encode<CS, SUB, 4, 4, true> : k_encode<CS, SUB, 2, 4, true>;
    if (mode == LUT_LINKEY_LDS)
        return vw == 4 ? k_encode<CS, SUB, 4, 7, true> : k_encode<CS, SUB, 2, 7, true>;
    if (mode == LUT_LITERAL_LDS)
        return k_encode<CS, SUB, 2, 0, true>;
    if (mode == LUT_LITERAL_GLOBAL)
        return k_encode<CS, SUB, 2, 2, true>;
    return nullptr;
}

namespace lhost {

enc_kernel_t pick_enc_f16(int cs, bool sub, int vw, int mode)
{
    switch (cs) {
    case CS_LUV: return sub ? pick_enc2_f16<CS_LUV, true>(vw, mode) : pick_enc2_f16<CS_LUV, false>(vw, mode);
    case CS_RGB: return sub ? pick_enc2_f16<CS_RGB, true>(vw, mode) : pick_enc2_f16<CS_RGB, false>(vw, mode);
    case CS_YCBCR: return sub ? pick_enc2_f16<CS_YCBCR, true>(vw, mode) : pick_enc2_f16<CS_YCBCR, false>(vw, mode);
    case CS_XYZ: return sub ? pick_enc2_f16<CS_XYZ, true>(vw, mode) : pick_enc2_f16<CS_XYZ, false>(vw, mode);
    }
    return nullptr;   // (CS_PACK: frames that are already colour-transformed are floats)
}

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
    const size_t n = (size_t)w * h;
    // (halves behind float pointers: the kernels read them as _Float16, all offsets count elements)
    const float *const pl[3] = {reinterpret_cast<const float *>(rgb), reinterpret_cast<const float *>(rgb + n),
                                reinterpret_cast<const float *>(rgb + 2 * n)};
    return encode_frames_device_impl(c, pl, frame_stride, nframes, w, h, sc, profile, planes, stride, pfs, stats, c->q.cs, true, IN16_TYPED);
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
    const float *const pl[3] = {reinterpret_cast<const float *>(rgb_planes[0]), reinterpret_cast<const float *>(rgb_planes[1]),
                                reinterpret_cast<const float *>(rgb_planes[2])};
    return encode_frames_device_impl(c, pl, frame_stride, nframes, w, h, sc, profile, planes, stride, pfs, stats, c->q.cs, true, IN16_TYPED);
}
