// lumahip_transcode.hip -- dispatch of the fused transcode kernels (lh::k_transcode, luma_kernels.hpp): code planes under the
// context's source quantizer -> code planes under its quantizer, no float frame between them.  Its own translation unit: the 48
// kernels compile side by side with the encode and decode units, and no kernel is in two code objects.  Also the plan of every
// launch over two plane sets (transcode_plan: the family's own part; what a measuring launch delivers and the checks every plan
// shares are lumahip_internal.hpp's) and, beside it, the one dispatch (measure_planes_impl) and the entry points of the five
// measuring calls over them, whose kernels lumahip_transcode_distortion.hip / lumahip_transcode_distortion_map.hip /
// lumahip_transcode_moments_map.hip / lumahip_transcode_half_distortion.hip / lumahip_transcode_half_distortion_map.hip compile.
#include "lumahip_internal.hpp"
#include "lumahip_pick.hpp"

using namespace lh;
using namespace lhost;

namespace lhost {

// The one place that decides what a launch over (source planes, target-side planes) may be and how it runs: argument checks, the
// supported set, the LDS budget, the kernel's key, vector width and launch shape -- for the transcode call (m == nullptr: tgt = the
// planes it writes; out = nullptr) and for the transcode distortion, the transcode distortion map and the transcode moments map (tgt =
// the given planes they read, out = their words; what differs between the three -- blocks accepted, words, LDS to meet in -- is the
// record's to say, the kernels' launch bound this plan's).  scale: 1, or 2 for the half-resolution transcode (lumahip_transcode_half.hip;
// m == nullptr) and for the half-resolution transcode distortion and its map (m built for w / 2 x h / 2): w x h is the source's size,
// the target side is (w / scale) x (h / scale) -- its layout, its extents, its geometry (p.e.g; p.d.g stays the source's), the
// vector width, the map's geometry and the grid, which runs over the target's tiles.  scale 4: the quarter-resolution transcode
// (lumahip_transcode_quarter.hip; m == nullptr only: no measuring call takes it), the same with (w / 4) x (h / 4).
int transcode_plan(lumahip_ctx *c, const SrcPlanes &src, float src_sc, unsigned nframes, unsigned w, unsigned h, const SrcPlanes &tgt, float dst_sc,
                   const MeasureOut *m, const uint64_t *out, hipStream_t stream, TranscodePlan &p, unsigned scale)
{
    const bool measure = m != nullptr, map = measure && m->map(), moments = measure && m->kind == DistWhat::Moments;
    const char *const what = measure ? m->call : "transcode";
    int rc;
    if ((measure && (rc = m->check_block(c))) || (rc = check_plane_sets(c, {{src}, {tgt}}, nframes != 0)))
        return rc;
    const int cse = c->q.cs;
    if ((rc = check_geom(c, w, h, tgt.profile, cse)))
        return rc;
    if (scale == 2 && ((w | h) & 3))
        return fail(c, LUMAHIP_ERR_ARG, "Invalid frame size %ux%u (half resolution: must be multiples of 4)", w, h);
    if (scale == 4 && ((w | h) & 7))
        return fail(c, LUMAHIP_ERR_ARG, "Invalid frame size %ux%u (quarter resolution: must be multiples of 8)", w, h);
    const unsigned tw = w / scale, th = h / scale;   // the target side's size
    if (src.profile < 0 || src.profile > 3)
        return fail(c, LUMAHIP_ERR_ARG, "source profile must be 0..3 (got %d)", src.profile);
    const lumahip_ctx::SourceQuant &sq = c->src;
    if (!sq.have)
        return fail(c, LUMAHIP_ERR_STATE, "source quantizer not set (call lumahip_set_source_quantizer first)");
    const int csd = sq.q.cs;
    if ((rc = check_planes_layout(c, src, nframes, w, h)) || (rc = check_planes_layout(c, tgt, nframes, tw, th)))
        return rc;
    if (!measure) {
        // no source plane may share a byte with a destination plane over the batch (the extent test of the rotating decode's buffers)
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++)
                if (ranges_overlap((uintptr_t)src.planes[i], plane_extent(w, h, src.profile, i, src.stride[i], src.pfs[i], nframes),
                                   (uintptr_t)tgt.planes[j], plane_extent(tw, th, tgt.profile, j, tgt.stride[j], tgt.pfs[j], nframes)))
                    return fail(c, LUMAHIP_ERR_ARG, "source plane %d and destination plane %d overlap over this batch", i, j);
    } else if ((rc = m->check_out(c, out)) || (rc = check_out_overlap(c, *m, out, nullptr, {{src, "source ", "", w, h}, {tgt, "given "}}))) {
        // (both plane sets are read only and may overlap each other; the words may not share a byte with anything the launch reads)
        return rc;
    }
    // ---- the supported set; everything else is refused here, before anything is launched
    if ((csd != CS_LUV && csd != CS_YCBCR) || (cse != CS_LUV && cse != CS_YCBCR))
        return fail(c, LUMAHIP_ERR_UNSUPPORTED, "%s: colour spaces Lu'v' and YCbCr only (source %d, target %d)", what, csd, cse);
    if (sq.bitdepth > 12 || !sq.lut_in_lds)
        return fail(c, LUMAHIP_ERR_UNSUPPORTED, "%s: the source's luminance table must be staged in LDS (bit depth <= 12, got %u)", what, sq.bitdepth);
    if (csd == CS_YCBCR && !sq.q.ytab)
        return fail(c, LUMAHIP_ERR_UNSUPPORTED, "%s: no y table for this YCbCr source (table values, LDS size or lumahip_tune \"ycbcr_tables\")", what);
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = ensure_search_index(c, stream)))
        return rc;
    const bool ycode = cse == CS_YCBCR;
    if (ycode ? !ycbcr_composite_ready(c) : (c->q.mode != LUT_THRESH_LDS && c->q.mode != LUT_LINKEY_LDS))
        return fail(c, LUMAHIP_ERR_UNSUPPORTED, "%s: the target needs %s in LDS (search mode %d)", what,
                    ycode ? "the composite luma -> code records" : "its luminance records", c->q.mode);
    const QuantDev &qe = ycode ? c->q_y : c->q;
    const bool any_y = csd == CS_YCBCR || cse == CS_YCBCR;
    const size_t col = round16(((size_t)sq.q.maxC + 1) * 4);
    // [powf tables once][source: luminance table + u'v' table | + y table + two chroma-term tables][target: records]  (k_transcode)
    const size_t lds = (any_y ? sizeof(PowfTablesWide) : 0) + lut_lds_bytes(sq.q) + (csd == CS_YCBCR ? lut_lds_bytes(sq.q) + 2 * col : col) +
                       round16((size_t)qe.nbuckets * (qe.mode == LUT_LINKEY_LDS ? 8 : 4));
    // the words the waves of a measuring workgroup meet in: 12, or the blocks of a map tile
    const size_t acc_lds = measure ? m->lds_bytes() : 0;
    if (lds + acc_lds > LUMAHIP_LDS_PER_WORKGROUP)
        return fail(c, LUMAHIP_ERR_UNSUPPORTED, "%s: the tables of both sides take %zu bytes of LDS, a workgroup has %zu", what, lds + acc_lds,
                    LUMAHIP_LDS_PER_WORKGROUP);

    p.csd = csd;
    p.cse = cse;
    p.subd = (src.profile == 0 || src.profile == 2);
    p.sube = (tgt.profile == 0 || tgt.profile == 2);
    p.any_y = any_y;
    p.kmode = ycode ? 5 : qe.mode;
    p.lds = lds;
    // four pixels per thread and row when every base and stride of both sides allows the vector accesses, else two
    p.vw = ((tw % 4) == 0 && planes_aligned(src, 4) && planes_aligned(tgt, 4)) ? 4 : 2;
    // (the half-resolution measuring kernels of some source families exist at VW 2 only: lh::transhalfdist_vw4)
    if (measure && scale == 2 && !transhalfdist_vw4(csd, p.subd, cse))
        p.vw = 2;
    // as the encode dispatch; the half-resolution Lu'v' -> Lu'v' kernels always: at VW 4 they are compiled for three waves per SIMD,
    // which three 256-thread workgroups per CU fill and one 512-thread workgroup does not (profiles/transcode_half_launch_shapes.txt);
    // the quarter-resolution ones, compiled for the same, likewise: 0.170 ms in three 256-thread workgroups per CU against 0.215 - 0.255 in
    // every other shape swept at 8 x 4K (profiles/transcode_quarter_launch_shapes.txt)
    const bool long_launch = scale != 1 || (unsigned long long)w * h * nframes >= 60000000ull;
    p.threads = block_threads_for(c, lds, long_launch && !any_y, any_y);
    // the measuring kernels are compiled for at most lh::TransDistBound threads (512 with YCbCr on either side, which is what the
    // rule above gives those pairs unless the tables or lumahip_tune "block" ask for more)
    // (the moments kernels: for lh::transmoments_threads_bound, the function their launch bound is written with)
    // (the half-resolution measuring kernels: for lh::transhalfdist_threads_bound / lh::transhalfmap_threads_bound, likewise)
    p.threads = std::min(p.threads, moments                 ? transmoments_threads_bound(csd, cse, p.vw)
                                    : measure && scale == 2 ? (map ? transhalfmap_threads_bound(csd, cse, p.vw) : transhalfdist_threads_bound(csd, cse, p.vw))
                                    : measure               ? TransDistFamily::bound(any_y)
                                    : scale == 2            ? transhalf_threads_bound(csd, cse, p.vw)
                                    : scale == 4            ? transquarter_threads_bound(csd, cse, p.vw)
                                                            : TransFamily::bound(any_y));
    if (map)
        p.threads = m->clamp_threads(p.threads);
    p.d = DecArgs{};
    p.e = EncArgs{};
    if (!make_geom(p.d.g, w, h, p.vw, p.threads / 64, nframes))
        return fail(c, LUMAHIP_ERR_ARG, "batch too large: more than 2^31 tiles in one launch");
    p.e.g = p.d.g;
    if (scale != 1)
        make_geom(p.e.g, tw, th, p.vw, p.threads / 64, nframes);   // (no larger and no more tiles than the source's: it cannot fail where that did not)
    p.d.q = sq.q;
    p.d.sc = src_sc;
    read_planes(p.d, src, p.vw);
    p.e.q = qe;
    p.e.q.cs = cse;
    p.e.sc = dst_sc;
    p.e.bps = tgt.profile > 1 ? 2 : 1;
    p.e.aligned = planes_aligned(tgt, p.vw) ? 1 : 0;
    p.grid = grid_for(c, p.threads, p.e.g.totalTiles, 0, 0, any_y ? 1 : 0, true);
    if (map)
        map_shape(*m, p.e.g, p.threads, p.m, p.grid);   // (the target side's geometry: the record's size)
    return LUMAHIP_OK;
}

int transcode_impl(lumahip_ctx *c, const SrcPlanes &src, float src_sc, unsigned nframes, unsigned w, unsigned h, const DstPlanes &dst, float dst_sc,
                   float *stats, const StreamLaunch &o)
{
    TranscodePlan p;
    int rc = transcode_plan(c, src, src_sc, nframes, w, h, {dst.planes, dst.stride, dst.pfs, dst.profile}, dst_sc, nullptr, nullptr, o.stream, p);
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
    const trans_kernel_t kern = p.vw == 4 ? pick_planes<TransFamily, 4>(p.csd, p.subd, p.cse, p.sube, p.kmode)
                                          : pick_planes<TransFamily, 2>(p.csd, p.subd, p.cse, p.sube, p.kmode);
    if (!kern)
        return fail(c, LUMAHIP_ERR_UNSUPPORTED, "no transcode kernel for colour spaces %d -> %d", p.csd, p.cse);
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

int measure_planes_impl(lumahip_ctx *c, const SrcPlanes &src, float src_sc, const SrcPlanes &given, float dst_sc, const MeasureOut &m, uint64_t *out,
                        const StreamLaunch &o, const SourceSize *full)
{
    TranscodePlan p;
    const bool half = full != nullptr;
    if (int rc = transcode_plan(c, src, src_sc, m.nframes, half ? full->w : m.w, half ? full->h : m.h, given, dst_sc, &m, out, o.stream, p,
                                half ? full->scale : 1))
        return rc;
    const auto no_kernel = [&] { return fail(c, LUMAHIP_ERR_UNSUPPORTED, "no %s kernel for colour spaces %d -> %d", m.call, p.csd, p.cse); };
    DecArgs g{};
    g.g = p.e.g;   // (the target side's geometry: the source's, or with `full` the half-size one)
    read_planes(g, given, p.vw);
    if (!m.map()) {
        TransDistArgs a{};
        a.d = p.d;
        a.e = p.e;
        a.g = g;
        a.out = out;
        const transdist_kernel_t kern = (half ? pick_transhalf_dist : pick_transdist)(p.vw, p.csd, p.subd, p.cse, p.sube, p.kmode);
        return kern ? launch_measure(c, m, out, kern, p.grid, p.threads, p.lds, launch_stream(c, o.stream, o.lanes), a) : no_kernel();
    }
    TransDistMapArgs a{};
    a.d = p.d;
    a.e = p.e;
    a.g = g;
    a.map = out;
    a.m = p.m;
    const transdist_map_kernel_t kern = (m.kind == DistWhat::Moments ? pick_transdist_moments_map : half ? pick_transhalf_dist_map : pick_transdist_map)(
        p.vw, p.csd, p.subd, p.cse, p.sube, p.kmode);
    return kern ? launch_measure(c, m, out, kern, p.grid, p.threads, p.lds, launch_stream(c, o.stream, o.lanes), a) : no_kernel();
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
    return device_entry(c, true, [&](const StreamLaunch &o) {
        return transcode_impl(c, {src_planes, src_stride, src_pfs, src_profile}, src_sc, nframes, w, h, {dst_planes, dst_stride, dst_pfs, dst_profile},
                              dst_sc, stats, o);
    });
}

// The five plane-fed measuring entry points (include/lumahip.h and, for the moments map, include/lumahip_measure.h, for the two
// half-resolution calls include/lumahip_ladder.h have their full prototypes): MEASURE_PARAMS, then the call's own tail.
#define MEASURE_PARAMS                                                                                                                      \
    const unsigned char *const src_planes[3], const int src_stride[3], const size_t src_pfs[3], int src_profile, float src_sc, unsigned nframes, \
        unsigned w, unsigned h, const unsigned char *const given_planes[3], const int given_stride[3], const size_t given_pfs[3], int dst_profile, \
        float dst_sc
#define CALL_Frame "transcode distortion"
#define CALL_Map "transcode distortion map"
#define CALL_Moments "transcode moments map"
// (the half-resolution calls: the record is the half-size target's, w x h stays the source's)
#define MEASURE_HALF(what, block, out)                                                                                                           \
    device_entry(c, true, [&](const StreamLaunch &o) {                                                                                           \
        const SourceSize full{w, h, 2};                                                                                                          \
        return measure_planes_impl(c, {src_planes, src_stride, src_pfs, src_profile}, src_sc, {given_planes, given_stride, given_pfs, dst_profile}, dst_sc, \
                                   {DistWhat::what, "half-resolution " CALL_##what, block, nframes, w / 2, h / 2}, out, o, &full);               \
    })
#define MEASURE(what, block, out)                                                                                                                \
    device_entry(c, true, [&](const StreamLaunch &o) {                                                                                           \
        return measure_planes_impl(c, {src_planes, src_stride, src_pfs, src_profile}, src_sc, {given_planes, given_stride, given_pfs, dst_profile}, dst_sc, \
                                   {DistWhat::what, CALL_##what, block, nframes, w, h}, out, o);                                                 \
    })
extern "C" {
int lumahip_transcode_distortion_frames_device(lumahip_ctx *c, MEASURE_PARAMS, uint64_t *out_dev) { return MEASURE(Frame, 0, out_dev); }
int lumahip_transcode_distortion_map_frames_device(lumahip_ctx *c, MEASURE_PARAMS, unsigned block, uint64_t *map_dev) { return MEASURE(Map, block, map_dev); }
int lumahip_transcode_moments_map_frames_device(lumahip_ctx *c, MEASURE_PARAMS, unsigned block, uint64_t *mom_dev) { return MEASURE(Moments, block, mom_dev); }
int lumahip_transcode_half_distortion_frames_device(lumahip_ctx *c, MEASURE_PARAMS, uint64_t *out_dev) { return MEASURE_HALF(Frame, 0, out_dev); }
int lumahip_transcode_half_distortion_map_frames_device(lumahip_ctx *c, MEASURE_PARAMS, unsigned block, uint64_t *map_dev) { return MEASURE_HALF(Map, block, map_dev); }
}  // extern "C"
