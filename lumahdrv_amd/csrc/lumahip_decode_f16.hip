// lumahip_decode_f16.hip -- the binary16-frame decode kernels (lh::k_decode<..., OUT16 = true>, luma_kernels.hpp), the C entry
// points lumahip_decode_frames_device_f16 / _planar_f16 and the narrowing probe.  Their own translation unit so that they
// compile side by side with the float kernels of lumahip_decode.hip.
#include "lumahip_internal.hpp"

using namespace lh;
using namespace lhost;

// The non-display choices of pick_dec2 (lumahip_decode.hip), with binary16 stores
template <int CS, bool SUB>
static dec_kernel_t pick_dec2_f16(int vw, bool gl, bool yt, bool rb)
{
    if constexpr (CS == CS_YCBCR) {
        if (yt && rb && !gl)
            return vw == 4 ? k_decode<CS, SUB, 4, false, false, true, true, true> : k_decode<CS, SUB, 2, false, false, true, true, true>;
        if (yt && !gl)
            return vw == 4 ? k_decode<CS, SUB, 4, false, false, true, false, true> : k_decode<CS, SUB, 2, false, false, true, false, true>;
    }
    if (gl)
        return k_decode<CS, SUB, 2, true, false, false, false, true>;
    return vw == 4 ? k_decode<CS, SUB, 4, false, false, false, false, true> : k_decode<CS, SUB, 2, false, false, false, false, true>;
}

namespace lhost {

dec_kernel_t pick_dec_f16(int cs, bool sub, int vw, bool gl, bool yt, bool rb)
{
    switch (cs) {
    case CS_LUV: return sub ? pick_dec2_f16<CS_LUV, true>(vw, gl, yt, rb) : pick_dec2_f16<CS_LUV, false>(vw, gl, yt, rb);
    case CS_RGB: return sub ? pick_dec2_f16<CS_RGB, true>(vw, gl, yt, rb) : pick_dec2_f16<CS_RGB, false>(vw, gl, yt, rb);
    case CS_YCBCR: return sub ? pick_dec2_f16<CS_YCBCR, true>(vw, gl, yt, rb) : pick_dec2_f16<CS_YCBCR, false>(vw, gl, yt, rb);
    case CS_XYZ: return sub ? pick_dec2_f16<CS_XYZ, true>(vw, gl, yt, rb) : pick_dec2_f16<CS_XYZ, false>(vw, gl, yt, rb);
    }
    return nullptr;   // (CS_PACK: the unpack-only decode writes dequantized floats; no _f16 entry point runs it)
}

}  // namespace lhost

extern "C" int lumahip_decode_frames_device_f16(lumahip_ctx *c, const unsigned char *const planes[3], const int stride[3],
                                                const size_t pfs[3], unsigned nframes, unsigned w, unsigned h, int profile,
                                                float sc, uint16_t *rgb, size_t frame_stride)
{
    if (!c)
        return LUMAHIP_ERR_ARG;
    if (!rgb)
        return fail(c, LUMAHIP_ERR_ARG, "null argument");
    if (!c->have_quant)
        return fail(c, LUMAHIP_ERR_STATE, "quantizer not set");
    const size_t n = (size_t)w * h;
    // (halves behind float pointers: the kernels store them as binary16, all offsets count elements)
    float *const pl[3] = {reinterpret_cast<float *>(rgb), reinterpret_cast<float *>(rgb + n), reinterpret_cast<float *>(rgb + 2 * n)};
    return decode_impl(c, planes, stride, pfs, nframes, w, h, profile, sc, pl, frame_stride, DisplayParams(), c->q.cs, true, nullptr, true);
}

extern "C" int lumahip_decode_frames_device_planar_f16(lumahip_ctx *c, const unsigned char *const planes[3], const int stride[3],
                                                       const size_t pfs[3], unsigned nframes, unsigned w, unsigned h, int profile,
                                                       float sc, uint16_t *const rgb_planes[3], size_t frame_stride)
{
    if (!c)
        return LUMAHIP_ERR_ARG;
    if (!rgb_planes || !rgb_planes[0])
        return fail(c, LUMAHIP_ERR_ARG, "null argument");
    if (!c->have_quant)
        return fail(c, LUMAHIP_ERR_STATE, "quantizer not set");
    float *const pl[3] = {reinterpret_cast<float *>(rgb_planes[0]), reinterpret_cast<float *>(rgb_planes[1]),
                          reinterpret_cast<float *>(rgb_planes[2])};
    return decode_impl(c, planes, stride, pfs, nframes, w, h, profile, sc, pl, frame_stride, DisplayParams(), c->q.cs, true, nullptr, true);
}

// ---- test probe: the decode kernels' narrowing (f16_narrow) of n consecutive fp32 bit patterns ----
namespace lh {
__global__ __launch_bounds__(256) void k_f16_narrow_probe(uint16_t *out, uint32_t first_bits, size_t n2)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (size_t)gridDim.x * blockDim.x) {
        float v[2] = {__uint_as_float(first_bits + (uint32_t)(2 * i)), __uint_as_float(first_bits + (uint32_t)(2 * i + 1))};
        store_px_h<2>(out + 2 * i, v);   // (the stores of k_decode<..., VW = 2, ..., OUT16>)
    }
}
}  // namespace lh

extern "C" int lumahip_f16_narrow_probe_device(lumahip_ctx *c, uint16_t *out_dev, uint32_t first_bits, size_t n)
{
    if (!c || !out_dev || n == 0 || (n % 2) != 0 || !is_aligned(out_dev, 4))
        return fail(c, LUMAHIP_ERR_ARG, "bad argument (n must be even, out 4-byte aligned)");
    HIPCHK(c, hipSetDevice(c->device));
    long grid = (long)((n / 2 + 255) / 256);
    if (grid > (long)c->num_cu * 8)
        grid = (long)c->num_cu * 8;
    hipLaunchKernelGGL(k_f16_narrow_probe, dim3((unsigned)grid), dim3(256), 0, c->stream, out_dev, first_bits, n / 2);
    HIPCHK(c, hipGetLastError());
    return LUMAHIP_OK;
}
