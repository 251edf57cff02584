// lumahip_distortion.hip -- dispatch of the code-domain distortion kernels (lh::k_distortion, luma_kernels.hpp): how far given code
// planes are from the planes lumahip_encode_frames_device would write for the same frames, as integer sums per frame and plane.
// Its own translation unit (float frames; lumahip_distortion_f16.hip holds the binary16-frame kernels): the kernels compile side
// by side with the encode, decode and transcode units, and no kernel is in two code objects.
#include "lumahip_internal.hpp"
#include "lumahip_pick.hpp"

using namespace lh;
using namespace lhost;

namespace lhost {

int distortion_impl(lumahip_ctx *c, const SrcFrames &f, float sc, const SrcPlanes &given, uint64_t *out, const DistortionLaunch &o)
{
    const bool in16 = f.elem == Elem::F16;
    const unsigned nframes = f.nframes, w = f.w, h = f.h;
    const int profile = given.profile;
    if (!f.plane[0] || !f.plane[1] || !f.plane[2] || !given.planes || !given.stride || !given.pfs || nframes == 0)
        return fail(c, LUMAHIP_ERR_ARG, "null argument");
    for (int p = 0; p < 3; p++)
        if (!given.planes[p])
            return fail(c, LUMAHIP_ERR_ARG, "null plane %d", p);
    const int cs = c->q.cs;
    int rc = check_geom(c, w, h, profile, cs);
    if (rc)
        return rc;
    if ((rc = check_layout(c, f, true, given.stride, given.pfs, profile)))
        return rc;
    if ((rc = check_out_words(c, out)))
        return rc;
    const size_t esz = elem_size(f.elem);
    bool al4;
    if ((rc = check_frame_alignment(c, f, esz, &al4)))
        return rc;
    // out_dev may not share a byte with anything the launch reads
    const size_t frame_span = ((size_t)(nframes - 1) * f.frame_stride + (size_t)w * h) * esz;
    for (int p = 0; p < 3; p++) {
        if (ranges_overlap((uintptr_t)out, out_words_bytes(nframes), (uintptr_t)f.plane[p], frame_span))
            return fail(c, LUMAHIP_ERR_ARG, "out_dev overlaps colour plane %d of the frames", p);
        if (out_overlaps_plane(out, given, p, w, h, nframes))
            return fail(c, LUMAHIP_ERR_ARG, "out_dev overlaps given plane %d", p);
    }
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = ensure_search_index(c, o.stream)))
        return rc;
    // ---- the supported set: the search records in LDS (the composite records of YCbCr exist only beside float-bit records in LDS)
    const int mode = c->q.mode;
    if (mode != LUT_THRESH_LDS && mode != LUT_LINKEY_LDS)
        return fail(c, LUMAHIP_ERR_UNSUPPORTED, "distortion: the search records must be in LDS (search mode %d)", mode);
    // the kernel, from the arguments alone: YCbCr float frames -> the composite records; YCbCr binary16 frames -> + the half-input
    // table whenever it exists for (sc, Lmax) and lumahip_tune("half_table") is not 0, else the general kernel (as the encode calls)
    bool ycode = !in16 && ycbcr_composite_ready(c);
    const float *half = nullptr;
    if (in16 && ycbcr_composite_ready(c) && c->half_mode != 0 && lds_bytes(c, true, cs, true, true) + 128 <= LUMAHIP_LDS_PER_WORKGROUP) {
        if ((rc = half_table_for(c, sc, &half)))
            return rc;
        ycode = half != nullptr;
    }
    const size_t lds = lds_bytes(c, true, cs, ycode, half != nullptr);
    if (lds + 128 > LUMAHIP_LDS_PER_WORKGROUP)   // (+ the 12 words the waves of a workgroup meet in)
        return fail(c, LUMAHIP_ERR_UNSUPPORTED, "distortion: the tables take %zu bytes of LDS, a workgroup has %zu", lds, LUMAHIP_LDS_PER_WORKGROUP);

    const bool sub = (profile == 0 || profile == 2);
    // four pixels per thread and row where the frames allow the 16 / 8-byte loads (the given planes fall back to byte loads by
    // themselves: DecArgs::aligned), else two
    const int vw = al4 ? 4 : 2;
    const bool long_launch = (unsigned long long)w * h * nframes >= 60000000ull;   // as the encode dispatch
    const int threads = block_threads_for(c, lds, long_launch && cs != CS_YCBCR, cs == CS_YCBCR && !half);
    DistArgs a{};
    if (!make_geom(a.e.g, w, h, vw, threads / 64, nframes))
        return fail(c, LUMAHIP_ERR_ARG, "batch too large: more than 2^31 tiles in one launch");
    a.g.g = a.e.g;
    a.e.q = ycode ? c->q_y : c->q;
    a.e.q.cs = cs;
    a.e.half = half;
    for (int k = 0; k < 3; k++)
        a.e.src[k] = static_cast<const float *>(f.plane[k]);   // (the IN16 kernels read the same pointers as halves: encode_frames_device_impl)
    a.e.frame_stride = f.frame_stride;
    a.e.sc = sc;
    read_planes(a.g, given, vw);
    a.e.bps = a.g.bps;
    a.out = out;
    const int kmode = half ? 6 : ycode ? 5 : mode;
    const dist_kernel_t kern = in16 ? pick_dist_f16(cs, sub, vw, kmode) : pick_dist<false>(cs, sub, vw, kmode);
    if (!kern)
        return fail(c, LUMAHIP_ERR_UNSUPPORTED, "no distortion kernel for colour space %d%s", cs, in16 ? " with binary16 frames" : "");
    const int grid = grid_for(c, threads, a.e.g.totalTiles, 0, 0, half ? 2 : cs == CS_YCBCR ? 1 : 0);
    return launch_measuring(c, kern, grid, threads, lds, launch_stream(c, o.stream, o.lanes), a, nframes);
}

}  // namespace lhost

extern "C" int lumahip_distortion_frames_device(lumahip_ctx *c, const float *rgb, size_t frame_stride, unsigned nframes, unsigned w, unsigned h,
                                                float sc, int profile, const unsigned char *const planes[3], const int stride[3],
                                                const size_t pfs[3], uint64_t *out_dev)
{
    if (!c)
        return LUMAHIP_ERR_ARG;
    if (!rgb)
        return fail(c, LUMAHIP_ERR_ARG, "null argument");
    return distortion_impl(c, packed_frames(rgb, frame_stride, nframes, w, h), sc, {planes, stride, pfs, profile}, out_dev, {c->stream, true});
}

extern "C" int lumahip_distortion_frames_device_planar(lumahip_ctx *c, const float *const rgb_planes[3], size_t frame_stride, unsigned nframes,
                                                       unsigned w, unsigned h, float sc, int profile, const unsigned char *const planes[3],
                                                       const int stride[3], const size_t pfs[3], uint64_t *out_dev)
{
    if (!c)
        return LUMAHIP_ERR_ARG;
    return distortion_impl(c, planar_frames(rgb_planes, frame_stride, nframes, w, h), sc, {planes, stride, pfs, profile}, out_dev,
                           {c->stream, true});
}
