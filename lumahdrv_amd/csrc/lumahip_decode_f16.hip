// lumahip_decode_f16.hip -- the binary16-frame decode kernels (lh::k_decode<..., OUT16 = true>, luma_kernels.hpp), the C entry
// points lumahip_decode_frames_device_f16 / _planar_f16 and the narrowing probe.  Their own translation unit so that they
// compile side by side with the float kernels of lumahip_decode.hip.
#include "lumahip_internal.hpp"
#include "lumahip_pick.hpp"

using namespace lh;
using namespace lhost;

namespace lhost {
dec_kernel_t pick_dec_f16(int cs, bool sub, int vw, bool gl, bool yt, bool rb) { return pick_dec<true>(cs, sub, vw, gl, false, yt, rb); }
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
    return decode_impl(c, {planes, stride, pfs, profile}, sc, packed_frames(rgb, frame_stride, nframes, w, h), {c->q.cs, c->stream, true});
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
    return decode_impl(c, {planes, stride, pfs, profile}, sc, planar_frames(rgb_planes, frame_stride, nframes, w, h), {c->q.cs, c->stream, true});
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
