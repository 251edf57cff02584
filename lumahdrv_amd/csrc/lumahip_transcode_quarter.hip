// lumahip_transcode_quarter.hip -- the quarter-resolution transcode kernels (lh::k_transcode_quarter, luma_kernels.hpp): code planes
// of w x h under the context's source quantizer -> code planes of (w/4) x (h/4) under its quantizer, the 2x2 box in linear light
// applied twice to floats between the decode and the encode, no float frame and no half-size planes.  Named here and nowhere else:
// their own translation unit, so that the 48 kernels compile side by side with the other units and no kernel is in two code objects.
// What a launch may be is transcode_plan's (lumahip_transcode.hip, scale 4); the dispatch and the _device entry point
// (include/lumahip_rungs.h) are here, the host form is lumahip_host.hip's.
#include "lumahip_internal.hpp"
#include "lumahip_pick.hpp"

using namespace lh;
using namespace lhost;

namespace lhost {

int transcode_quarter_impl(lumahip_ctx *c, const SrcPlanes &src, float src_sc, unsigned nframes, unsigned w, unsigned h, const DstPlanes &dst, float dst_sc,
                           float *stats, const StreamLaunch &o)
{
    TranscodePlan p;
    int rc = transcode_plan(c, src, src_sc, nframes, w, h, {dst.planes, dst.stride, dst.pfs, dst.profile}, dst_sc, nullptr, nullptr, o.stream, p, 4);
    if (rc)
        return rc;
    TransArgs a{};
    a.d = p.d;
    a.e = p.e;
    for (int k = 0; k < 3; k++) {
        a.e.dst[k] = dst.planes[k];
        a.e.stride[k] = dst.stride[k];
        a.e.dst_frame_stride[k] = dst.pfs[k];
    }
    const trans_kernel_t kern = p.vw == 4 ? pick_planes<TransQuarterFamily, 4>(p.csd, p.subd, p.cse, p.sube, p.kmode)
                                          : pick_planes<TransQuarterFamily, 2>(p.csd, p.subd, p.cse, p.sube, p.kmode);
    if (!kern)
        return fail(c, LUMAHIP_ERR_UNSUPPORTED, "no quarter-resolution transcode kernel for colour spaces %d -> %d", p.csd, p.cse);
    hipStream_t s = launch_stream(c, o.stream, o.lanes);
    if (stats && (rc = stats_begin(c, nframes, o.lanes, &s, &a.e.stats)))
        return rc;
    if ((rc = launch_fused(c, kern, p.grid, p.threads, p.lds, s, a)))
        return rc;
    if (stats)
        stats_fold(c, nframes, stats, s);
    HIPCHK(c, hipGetLastError());
    return LUMAHIP_OK;
}

}  // namespace lhost

extern "C" int lumahip_transcode_quarter_frames_device(lumahip_ctx *c, const unsigned char *const src_planes[3], const int src_stride[3],
                                                       const size_t src_pfs[3], int src_profile, float src_sc, unsigned nframes, unsigned w, unsigned h,
                                                       unsigned char *const dst_planes[3], const int dst_stride[3], const size_t dst_pfs[3],
                                                       int dst_profile, float dst_sc, float *stats)
{
    return device_entry(c, true, [&](const StreamLaunch &o) {
        return transcode_quarter_impl(c, {src_planes, src_stride, src_pfs, src_profile}, src_sc, nframes, w, h,
                                      {dst_planes, dst_stride, dst_pfs, dst_profile}, dst_sc, stats, o);
    });
}
