// lumahip_transcode.hip -- dispatch of the fused transcode kernels (lh::k_transcode, luma_kernels.hpp): code planes under the
// context's source quantizer -> code planes under its quantizer, no float frame between them.  Its own translation unit: the 48
// kernels compile side by side with the encode and decode units, and no kernel is in two code objects.
#include "lumahip_internal.hpp"
#include "lumahip_pick.hpp"

using namespace lh;
using namespace lhost;

namespace lhost {

static size_t round16(size_t b) { return (b + 15) & ~(size_t)15; }

int transcode_impl(lumahip_ctx *c, const SrcPlanes &src, float src_sc, unsigned nframes, unsigned w, unsigned h, const DstPlanes &dst, float dst_sc,
                   float *stats, const TranscodeLaunch &o)
{
    if (!src.planes || !src.stride || !src.pfs || !dst.planes || !dst.stride || !dst.pfs || nframes == 0)
        return fail(c, LUMAHIP_ERR_ARG, "null argument");
    for (int p = 0; p < 3; p++)
        if (!src.planes[p] || !dst.planes[p])
            return fail(c, LUMAHIP_ERR_ARG, "null plane %d", p);
    const int cse = c->q.cs;
    int rc = check_geom(c, w, h, dst.profile, cse);
    if (rc)
        return rc;
    if (src.profile < 0 || src.profile > 3)
        return fail(c, LUMAHIP_ERR_ARG, "source profile must be 0..3 (got %d)", src.profile);
    const lumahip_ctx::SourceQuant &sq = c->src;
    if (!sq.have)
        return fail(c, LUMAHIP_ERR_STATE, "source quantizer not set (call lumahip_set_source_quantizer first)");
    const int csd = sq.q.cs;
    const SrcFrames geom{{nullptr, nullptr, nullptr}, Elem::F32, 0, nframes, w, h};   // (the code planes' checks read the geometry only)
    if ((rc = check_layout(c, geom, false, src.stride, src.pfs, src.profile)) || (rc = check_layout(c, geom, false, dst.stride, dst.pfs, dst.profile)))
        return rc;
    // no source plane may share a byte with a destination plane over the batch (the extent test of the rotating decode's buffers)
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            const uintptr_t bi = (uintptr_t)src.planes[i], bj = (uintptr_t)dst.planes[j];
            const size_t ei = plane_extent(w, h, src.profile, i, src.stride[i], src.pfs[i], nframes);
            const size_t ej = plane_extent(w, h, dst.profile, j, dst.stride[j], dst.pfs[j], nframes);
            if (bi < bj + ej && bj < bi + ei)
                return fail(c, LUMAHIP_ERR_ARG, "source plane %d and destination plane %d overlap over this batch", i, j);
        }
    // ---- the supported set; everything else is refused here, before anything is launched
    if ((csd != CS_LUV && csd != CS_YCBCR) || (cse != CS_LUV && cse != CS_YCBCR))
        return fail(c, LUMAHIP_ERR_UNSUPPORTED, "transcode: colour spaces Lu'v' and YCbCr only (source %d, target %d)", csd, cse);
    if (sq.bitdepth > 12 || !sq.lut_in_lds)
        return fail(c, LUMAHIP_ERR_UNSUPPORTED, "transcode: the source's luminance table must be staged in LDS (bit depth <= 12, got %u)", sq.bitdepth);
    if (csd == CS_YCBCR && !sq.q.ytab)
        return fail(c, LUMAHIP_ERR_UNSUPPORTED, "transcode: no y table for this YCbCr source (table values, LDS size or lumahip_tune \"ycbcr_tables\")");
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = ensure_search_index(c, o.stream)))
        return rc;
    const bool ycode = cse == CS_YCBCR;
    if (ycode ? !ycbcr_composite_ready(c) : (c->q.mode != LUT_THRESH_LDS && c->q.mode != LUT_LINKEY_LDS))
        return fail(c, LUMAHIP_ERR_UNSUPPORTED, "transcode: the target needs %s in LDS (search mode %d)",
                    ycode ? "the composite luma -> code records" : "its luminance records", c->q.mode);
    const QuantDev &qe = ycode ? c->q_y : c->q;
    const bool any_y = csd == CS_YCBCR || cse == CS_YCBCR;
    const size_t col = round16(((size_t)sq.q.maxC + 1) * 4);
    // [powf tables once][source: luminance table + u'v' table | + y table + two chroma-term tables][target: records]  (k_transcode)
    const size_t lds = (any_y ? sizeof(PowfTablesWide) : 0) + lut_lds_bytes(sq.q) + (csd == CS_YCBCR ? lut_lds_bytes(sq.q) + 2 * col : col) +
                       round16((size_t)qe.nbuckets * (qe.mode == LUT_LINKEY_LDS ? 8 : 4));
    if (lds > LUMAHIP_LDS_PER_WORKGROUP)
        return fail(c, LUMAHIP_ERR_UNSUPPORTED, "transcode: the tables of both sides take %zu bytes of LDS, a workgroup has %zu", lds, LUMAHIP_LDS_PER_WORKGROUP);

    const bool subd = (src.profile == 0 || src.profile == 2), sube = (dst.profile == 0 || dst.profile == 2);
    // four pixels per thread and row when every base and stride of both sides allows the vector accesses, else two
    const int vw = ((w % 4) == 0 && planes_aligned(src, 4) && planes_aligned(dst, 4)) ? 4 : 2;
    const bool long_launch = (unsigned long long)w * h * nframes >= 60000000ull;   // as the encode dispatch
    const int threads = block_threads_for(c, lds, long_launch && !any_y, any_y);
    TransArgs a{};
    if (!make_geom(a.d.g, w, h, vw, threads / 64, nframes))
        return fail(c, LUMAHIP_ERR_ARG, "batch too large: more than 2^31 tiles in one launch");
    a.e.g = a.d.g;
    a.d.q = sq.q;
    a.e.q = qe;
    a.e.q.cs = cse;
    a.d.sc = src_sc;
    a.e.sc = dst_sc;
    a.d.bps = src.profile > 1 ? 2 : 1;
    a.e.bps = dst.profile > 1 ? 2 : 1;
    a.d.aligned = planes_aligned(src, vw) ? 1 : 0;
    a.e.aligned = planes_aligned(dst, vw) ? 1 : 0;
    for (int p = 0; p < 3; p++) {
        a.d.src[p] = src.planes[p];
        a.d.stride[p] = src.stride[p];
        a.d.src_frame_stride[p] = src.pfs[p];
        a.e.dst[p] = dst.planes[p];
        a.e.stride[p] = dst.stride[p];
        a.e.dst_frame_stride[p] = dst.pfs[p];
    }
    const trans_kernel_t kern = vw == 4 ? pick_trans<4>(csd, subd, cse, sube, ycode ? 5 : qe.mode) : pick_trans<2>(csd, subd, cse, sube, ycode ? 5 : qe.mode);
    if (!kern)
        return fail(c, LUMAHIP_ERR_UNSUPPORTED, "no transcode kernel for colour spaces %d -> %d", csd, cse);
    if (lds > 64 * 1024)
        HIPCHK(c, hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int grid = grid_for(c, threads, a.d.g.totalTiles, 0, 0, any_y ? 1 : 0, true);
    hipStream_t s = launch_stream(c, o.stream, o.lanes);
    if (stats && (rc = stats_begin(c, nframes, o.lanes, &s, &a.e.stats)))
        return rc;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), lds, s, a);
    if (stats)
        stats_fold(c, nframes, stats, s);
    HIPCHK(c, hipGetLastError());
    return LUMAHIP_OK;
}

// channel 0 of the decoded and colour-transformed frame (one frame, planes without a frame stride) into out_dev, w*h floats
int transcode_channel0(lumahip_ctx *c, const SrcPlanes &src, float src_sc, unsigned w, unsigned h, float dst_sc, float *out_dev, hipStream_t s)
{
    const lumahip_ctx::SourceQuant &sq = c->src;
    TransChan0Args a{};
    a.qd = sq.q;
    for (int p = 0; p < 3; p++) {
        a.src[p] = src.planes[p];
        a.stride[p] = src.stride[p];
    }
    a.bps = src.profile > 1 ? 2 : 1;
    a.sub = (src.profile == 0 || src.profile == 2) ? 1 : 0;
    a.w = (int)w;
    a.h = (int)h;
    a.sc_src = src_sc;
    a.sc_dst = dst_sc;
    a.Lmax_dst = c->q.Lmax;
    a.out = out_dev;
    void (*kern)(const TransChan0Args) = nullptr;
    const int csd = sq.q.cs, cse = c->q.cs;
    if (csd == CS_LUV)
        kern = cse == CS_LUV ? k_transcode_channel0<CS_LUV, CS_LUV> : k_transcode_channel0<CS_LUV, CS_YCBCR>;
    else
        kern = cse == CS_LUV ? k_transcode_channel0<CS_YCBCR, CS_LUV> : k_transcode_channel0<CS_YCBCR, CS_YCBCR>;
    hipLaunchKernelGGL(kern, dim3((unsigned)c->num_cu * 8), dim3(256), 0, s, a);
    HIPCHK(c, hipGetLastError());
    return LUMAHIP_OK;
}

}  // namespace lhost

extern "C" int lumahip_transcode_frames_device(lumahip_ctx *c, const unsigned char *const src_planes[3], const int src_stride[3],
                                               const size_t src_pfs[3], int src_profile, float src_sc, unsigned nframes, unsigned w, unsigned h,
                                               unsigned char *const dst_planes[3], const int dst_stride[3], const size_t dst_pfs[3],
                                               int dst_profile, float dst_sc, float *stats)
{
    if (!c)
        return LUMAHIP_ERR_ARG;
    return transcode_impl(c, {src_planes, src_stride, src_pfs, src_profile}, src_sc, nframes, w, h, {dst_planes, dst_stride, dst_pfs, dst_profile}, dst_sc,
                          stats, {c->stream, true});
}
