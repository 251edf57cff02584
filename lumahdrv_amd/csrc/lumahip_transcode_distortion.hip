// lumahip_transcode_distortion.hip -- dispatch of the transcode distortion kernels (lh::k_transcode_distortion, luma_kernels.hpp): how
// far given code planes are from the planes lumahip_transcode_frames_device would write for the same source planes, as integer
// sums per frame and plane.  What the launch may be and how it runs is transcode_plan's decision (lumahip_transcode.hip), shared
// with the transcode call.  Its own translation unit: the 48 kernels compile side by side with the other units, and no kernel is
// in two code objects.
#include "lumahip_internal.hpp"
#include "lumahip_pick.hpp"

using namespace lh;
using namespace lhost;

namespace lhost {

int transcode_distortion_impl(lumahip_ctx *c, const SrcPlanes &src, float src_sc, unsigned nframes, unsigned w, unsigned h, const SrcPlanes &given,
                              float dst_sc, uint64_t *out, const TranscodeLaunch &o)
{
    TranscodePlan p;
    int rc = transcode_plan(c, src, src_sc, nframes, w, h, given, dst_sc, true, out, o.stream, p);
    if (rc)
        return rc;
    TransDistArgs a{};
    a.d = p.d;
    a.e = p.e;
    a.g.g = p.d.g;
    a.g.bps = p.e.bps;
    a.g.aligned = p.e.aligned;
    for (int k = 0; k < 3; k++) {
        a.g.src[k] = given.planes[k];
        a.g.stride[k] = given.stride[k];
        a.g.src_frame_stride[k] = given.pfs[k];
    }
    a.out = out;
    int bound = 0;
    const transdist_kernel_t kern = p.vw == 4 ? pick_transdist<4>(p.csd, p.subd, p.cse, p.sube, p.kmode, &bound)
                                              : pick_transdist<2>(p.csd, p.subd, p.cse, p.sube, p.kmode, &bound);
    if (!kern)
        return fail(c, LUMAHIP_ERR_UNSUPPORTED, "no transcode distortion kernel for colour spaces %d -> %d", p.csd, p.cse);
    if (p.threads > bound)   // (transcode_plan clamps to the same constants: never taken)
        return fail(c, LUMAHIP_ERR_UNSUPPORTED, "transcode distortion: %d threads per workgroup, the kernel takes %d", p.threads, bound);
    if (p.lds > 64 * 1024)
        HIPCHK(c, hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds));
    hipStream_t s = launch_stream(c, o.stream, o.lanes);
    HIPCHK(c, hipMemsetAsync(out, 0, (size_t)nframes * 12 * sizeof(uint64_t), s));
    hipLaunchKernelGGL(kern, dim3(p.grid), dim3(p.threads), p.lds, s, a);
    HIPCHK(c, hipGetLastError());
    return LUMAHIP_OK;
}

}  // namespace lhost

extern "C" int lumahip_transcode_distortion_frames_device(lumahip_ctx *c, const unsigned char *const src_planes[3], const int src_stride[3],
                                                          const size_t src_pfs[3], int src_profile, float src_sc, unsigned nframes, unsigned w,
                                                          unsigned h, const unsigned char *const given_planes[3], const int given_stride[3],
                                                          const size_t given_pfs[3], int dst_profile, float dst_sc, uint64_t *out_dev)
{
    if (!c)
        return LUMAHIP_ERR_ARG;
    return transcode_distortion_impl(c, {src_planes, src_stride, src_pfs, src_profile}, src_sc, nframes, w, h,
                                     {given_planes, given_stride, given_pfs, dst_profile}, dst_sc, out_dev, {c->stream, true});
}
