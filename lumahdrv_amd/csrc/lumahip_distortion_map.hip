// lumahip_distortion_map.hip -- dispatch of the distortion map kernels (lh::k_distortion_map, luma_kernels.hpp): what
// lumahip_distortion_frames_device sums per frame, per block of 16, 32 or 64 luma pixels squared, every word of the map written once
// by one launch.  Its own translation unit (float frames; lumahip_distortion_map_f16.hip holds the binary16-frame kernels): the
// kernels compile side by side with the other units', and no kernel is in two code objects.
#include "lumahip_internal.hpp"
#include "lumahip_pick.hpp"

using namespace lh;
using namespace lhost;

namespace lhost {

int distortion_map_impl(lumahip_ctx *c, const SrcFrames &f, float sc, const SrcPlanes &given, unsigned block, uint64_t *map, const DistortionLaunch &o)
{
    DistortionPlan p;
    if (int rc = distortion_plan(c, f, sc, given, map, DistWhat::Map, block, o.stream, p))
        return rc;
    DistMapArgs a{};
    a.e = p.e;
    a.g = p.g;
    a.map = map;
    a.m = make_map_geom(p.e.g, f.w, f.h, block, p.threads);   // (S >= 1: distortion_plan has clamped the workgroup)
    const dist_map_kernel_t kern = p.in16 ? pick_dist_map_f16(p.cs, p.sub, p.vw, p.kmode) : pick_dist<DistMapFamily, false>(p.cs, p.sub, p.vw, p.kmode);
    if (!kern)
        return fail(c, LUMAHIP_ERR_UNSUPPORTED, "no distortion map kernel for colour space %d%s", p.cs, p.in16 ? " with binary16 frames" : "");
    // grid_for's encode rule over the standard tiles; a workgroup takes whole map tiles
    const int grid = p.grid < a.m.totalMapTiles ? p.grid : a.m.totalMapTiles;
    if (int rc = launch_fused(c, kern, grid, p.threads, p.lds, launch_stream(c, o.stream, o.lanes), a))
        return rc;
    HIPCHK(c, hipGetLastError());
    return LUMAHIP_OK;
}

}  // namespace lhost

extern "C" int lumahip_distortion_map_dims(unsigned w, unsigned h, unsigned block, unsigned *nbx, unsigned *nby)
{
    if (!dist_map_block_ok(block) || !nbx || !nby)
        return LUMAHIP_ERR_ARG;
    *nbx = (w + block - 1) / block;
    *nby = (h + block - 1) / block;
    return LUMAHIP_OK;
}

extern "C" int lumahip_distortion_map_frames_device(lumahip_ctx *c, const float *rgb, size_t frame_stride, unsigned nframes, unsigned w, unsigned h,
                                                    float sc, int profile, const unsigned char *const planes[3], const int stride[3],
                                                    const size_t pfs[3], unsigned block, uint64_t *map_dev)
{
    if (!c)
        return LUMAHIP_ERR_ARG;
    if (!rgb)
        return fail(c, LUMAHIP_ERR_ARG, "null argument");
    return distortion_map_impl(c, packed_frames(rgb, frame_stride, nframes, w, h), sc, {planes, stride, pfs, profile}, block, map_dev,
                               {c->stream, true});
}

extern "C" int lumahip_distortion_map_frames_device_planar(lumahip_ctx *c, const float *const rgb_planes[3], size_t frame_stride, unsigned nframes,
                                                           unsigned w, unsigned h, float sc, int profile, const unsigned char *const planes[3],
                                                           const int stride[3], const size_t pfs[3], unsigned block, uint64_t *map_dev)
{
    if (!c)
        return LUMAHIP_ERR_ARG;
    return distortion_map_impl(c, planar_frames(rgb_planes, frame_stride, nframes, w, h), sc, {planes, stride, pfs, profile}, block, map_dev,
                               {c->stream, true});
}
