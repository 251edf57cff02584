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
    int rc = transcode_plan(c, src, src_sc, nframes, w, h, given, dst_sc, TransWhat::Measure, out, 0, o.stream, p);
    if (rc)
        return rc;
    TransDistArgs a{};
    a.d = p.d;
    a.e = p.e;
    a.g.g = p.d.g;
    read_planes(a.g, given, p.vw);
    a.out = out;
    const transdist_kernel_t kern = p.vw == 4 ? pick_planes<TransDistFamily, 4>(p.csd, p.subd, p.cse, p.sube, p.kmode)
                                              : pick_planes<TransDistFamily, 2>(p.csd, p.subd, p.cse, p.sube, p.kmode);
    if (!kern)
        return fail(c, LUMAHIP_ERR_UNSUPPORTED, "no transcode distortion kernel for colour spaces %d -> %d", p.csd, p.cse);
    return launch_measuring(c, kern, p.grid, p.threads, p.lds, launch_stream(c, o.stream, o.lanes), a, nframes);
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
