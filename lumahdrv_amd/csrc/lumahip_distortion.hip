// lumahip_distortion.hip -- the frame-fed measuring calls: how far given code planes are from the planes lumahip_encode_frames_device
// would write for the same frames, as integer sums per frame and plane (lh::k_distortion, luma_kernels.hpp), per block (k_distortion_map)
// or as the moments of both signals per block (k_moments_map).  One plan (distortion_plan: what is this family's own -- the quantizer it
// needs, its supported set and LDS budget, vector width, workgroup and grid; the rest is lumahip_internal.hpp's MeasureOut and shared
// checks), one dispatch (measure_frames_impl) and the entry points of all three; of the kernels this unit compiles the float-frame
// k_distortion only.  The others have a translation unit each that exports their picker (lumahip_distortion_f16.hip,
// lumahip_distortion_map.hip / _f16.hip, lumahip_moments_map.hip / _f16.hip): they compile side by side, and no kernel is in two
// code objects.
#include "lumahip_internal.hpp"
#include "lumahip_pick.hpp"

using namespace lh;
using namespace lhost;

namespace lhost {

int distortion_plan(lumahip_ctx *c, const SrcFrames &f, float sc, const SrcPlanes &given, const MeasureOut &m, const uint64_t *out,
                    hipStream_t stream, DistortionPlan &p)
{
    const char *const what = m.call;
    const DistWhat kind = m.kind;
    int rc = m.check_block(c);
    if (rc)
        return rc;
    const bool in16 = f.elem == Elem::F16;
    const unsigned nframes = f.nframes, w = f.w, h = f.h;
    const int profile = given.profile;
    if ((rc = check_plane_sets(c, {{given}}, f.plane[0] && f.plane[1] && f.plane[2] && nframes != 0)))
        return rc;
    const int cs = c->q.cs;
    if ((rc = check_geom(c, w, h, profile, cs)) || (rc = check_layout(c, f, true, given.stride, given.pfs, profile)) || (rc = m.check_out(c, out)))
        return rc;
    bool al4;
    if ((rc = check_frame_alignment(c, f, elem_size(f.elem), &al4)) || (rc = check_out_overlap(c, m, out, &f, {{given, "given "}})))
        return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = ensure_search_index(c, stream)))
        return rc;
    // ---- the supported set: the search records in LDS (the composite records of YCbCr exist only beside float-bit records in LDS)
    const int mode = c->q.mode;
    if (mode != LUT_THRESH_LDS && mode != LUT_LINKEY_LDS)
        return fail(c, LUMAHIP_ERR_UNSUPPORTED, "%s: the search records must be in LDS (search mode %d)", what, mode);
    // the kernel, from the arguments alone: YCbCr float frames -> the composite records; YCbCr binary16 frames -> + the half-input
    // table whenever it exists for (sc, Lmax) and lumahip_tune("half_table") is not 0, else the general kernel (as the encode calls)
    bool ycode = !in16 && ycbcr_composite_ready(c);
    const float *half = nullptr;
    // (+ the words the waves of a workgroup meet in: 12, or the blocks of a map tile)
    const size_t meet = m.lds_bytes();
    if (in16 && ycbcr_composite_ready(c) && c->half_mode != 0 && lds_bytes(c, true, cs, true, true) + meet <= LUMAHIP_LDS_PER_WORKGROUP) {
        if ((rc = half_table_for(c, sc, &half)))
            return rc;
        ycode = half != nullptr;
    }
    const size_t lds = lds_bytes(c, true, cs, ycode, half != nullptr);
    if (lds + meet > LUMAHIP_LDS_PER_WORKGROUP)
        return fail(c, LUMAHIP_ERR_UNSUPPORTED, "%s: the tables take %zu bytes of LDS, a workgroup has %zu", what, lds, LUMAHIP_LDS_PER_WORKGROUP);

    p.cs = cs;
    p.in16 = in16;
    p.sub = (profile == 0 || profile == 2);
    // four pixels per thread and row where the frames allow the 16 / 8-byte loads (the given planes fall back to byte loads by
    // themselves: DecArgs::aligned), else two
    p.vw = al4 ? 4 : 2;
    const bool long_launch = (unsigned long long)w * h * nframes >= 60000000ull;   // as the encode dispatch
    p.threads = block_threads_for(c, lds, long_launch && cs != CS_YCBCR, cs == CS_YCBCR && !half);
    p.threads = m.clamp_threads(p.threads);
    p.kmode = half ? 6 : ycode ? 5 : mode;
    // ... and the moments kernels that are register-allocated for fewer threads run with at most those
    if (kind == DistWhat::Moments && p.threads > moments_threads_bound(cs, p.sub, p.vw, p.kmode))
        p.threads = moments_threads_bound(cs, p.sub, p.vw, p.kmode);
    p.lds = lds;
    p.e = EncArgs{};
    p.g = DecArgs{};
    if (!make_geom(p.e.g, w, h, p.vw, p.threads / 64, nframes))
        return fail(c, LUMAHIP_ERR_ARG, "batch too large: more than 2^31 tiles in one launch");
    p.g.g = p.e.g;
    p.e.q = ycode ? c->q_y : c->q;
    p.e.q.cs = cs;
    p.e.half = half;
    for (int k = 0; k < 3; k++)
        p.e.src[k] = static_cast<const float *>(f.plane[k]);   // (the IN16 kernels read the same pointers as halves: encode_frames_device_impl)
    p.e.frame_stride = f.frame_stride;
    p.e.sc = sc;
    read_planes(p.g, given, p.vw);
    p.e.bps = p.g.bps;
    // grid_for's encode rule over the standard tiles
    p.grid = grid_for(c, p.threads, p.e.g.totalTiles, 0, 0, half ? 2 : cs == CS_YCBCR ? 1 : 0);
    map_shape(m, p.e.g, p.threads, p.m, p.grid);   // (S >= 1: the workgroup is clamped above)
    return LUMAHIP_OK;
}

dist_kernel_t pick_dist_f32(int cs, bool sub, int vw, int mode) { return pick_dist<DistFamily, false>(cs, sub, vw, mode); }

int measure_frames_impl(lumahip_ctx *c, const SrcFrames &f, float sc, const SrcPlanes &given, const MeasureOut &m, uint64_t *out,
                        const StreamLaunch &o)
{
    DistortionPlan p;
    if (int rc = distortion_plan(c, f, sc, given, m, out, o.stream, p))
        return rc;
    const auto no_kernel = [&] {
        return fail(c, LUMAHIP_ERR_UNSUPPORTED, "no %s kernel for colour space %d%s", m.call, p.cs, p.in16 ? " with binary16 frames" : "");
    };
    if (!m.map()) {
        DistArgs a{};
        a.e = p.e;
        a.g = p.g;
        a.out = out;
        const dist_kernel_t kern = (p.in16 ? pick_dist_f16 : pick_dist_f32)(p.cs, p.sub, p.vw, p.kmode);
        return kern ? launch_measure(c, m, out, kern, p.grid, p.threads, p.lds, launch_stream(c, o.stream, o.lanes), a) : no_kernel();
    }
    MapArgs a{};
    a.e = p.e;
    a.g = p.g;
    a.map = out;
    a.m = p.m;
    const map_kernel_t kern = (m.kind == DistWhat::Moments ? (p.in16 ? pick_moments_map_f16 : pick_moments_map_f32)
                                                           : (p.in16 ? pick_dist_map_f16 : pick_dist_map_f32))(p.cs, p.sub, p.vw, p.kmode);
    return kern ? launch_measure(c, m, out, kern, p.grid, p.threads, p.lds, launch_stream(c, o.stream, o.lanes), a) : no_kernel();
}

static int map_dims(DistWhat what, unsigned w, unsigned h, unsigned block, unsigned *nbx, unsigned *nby)
{
    const MeasureOut m(what, "", block, 1, w, h);
    if (!m.block_ok() || !nbx || !nby)
        return LUMAHIP_ERR_ARG;
    *nbx = m.nbx();
    *nby = m.nby();
    return LUMAHIP_OK;
}

}  // namespace lhost

// The twelve _device entry points and the two *_map_dims (include/lumahip.h has their full prototypes): the frames, MEASURE_PARAMS,
// then the call's own tail.
#define MEASURE_PARAMS                                                                                                                   \
    size_t frame_stride, unsigned nframes, unsigned w, unsigned h, float sc, int profile, const unsigned char *const planes[3],         \
        const int stride[3], const size_t pfs[3]
#define CALL_Frame "distortion"
#define CALL_Map "distortion map"
#define CALL_Moments "moments map"
#define ENTRY(given, frames, what, block, out)                                                                                          \
    device_entry(c, given, [&](const StreamLaunch &o) {                                                                                \
        return measure_frames_impl(c, frames, sc, {planes, stride, pfs, profile}, {DistWhat::what, CALL_##what, block, nframes, w, h}, out, o); \
    })
#define PACKED(what, block, out) ENTRY(rgb != nullptr, packed_frames(rgb, frame_stride, nframes, w, h), what, block, out)
#define PLANAR(what, block, out) ENTRY(true, planar_frames(rgb_planes, frame_stride, nframes, w, h), what, block, out)
extern "C" {
int lumahip_distortion_frames_device(lumahip_ctx *c, const float *rgb, MEASURE_PARAMS, uint64_t *out_dev) { return PACKED(Frame, 0, out_dev); }
int lumahip_distortion_frames_device_planar(lumahip_ctx *c, const float *const rgb_planes[3], MEASURE_PARAMS, uint64_t *out_dev) { return PLANAR(Frame, 0, out_dev); }
int lumahip_distortion_frames_device_f16(lumahip_ctx *c, const uint16_t *rgb, MEASURE_PARAMS, uint64_t *out_dev) { return PACKED(Frame, 0, out_dev); }
int lumahip_distortion_frames_device_planar_f16(lumahip_ctx *c, const uint16_t *const rgb_planes[3], MEASURE_PARAMS, uint64_t *out_dev) { return PLANAR(Frame, 0, out_dev); }

int lumahip_distortion_map_dims(unsigned w, unsigned h, unsigned block, unsigned *nbx, unsigned *nby) { return map_dims(DistWhat::Map, w, h, block, nbx, nby); }
int lumahip_distortion_map_frames_device(lumahip_ctx *c, const float *rgb, MEASURE_PARAMS, unsigned block, uint64_t *map_dev) { return PACKED(Map, block, map_dev); }
int lumahip_distortion_map_frames_device_planar(lumahip_ctx *c, const float *const rgb_planes[3], MEASURE_PARAMS, unsigned block, uint64_t *map_dev) { return PLANAR(Map, block, map_dev); }
int lumahip_distortion_map_frames_device_f16(lumahip_ctx *c, const uint16_t *rgb, MEASURE_PARAMS, unsigned block, uint64_t *map_dev) { return PACKED(Map, block, map_dev); }
int lumahip_distortion_map_frames_device_planar_f16(lumahip_ctx *c, const uint16_t *const rgb_planes[3], MEASURE_PARAMS, unsigned block, uint64_t *map_dev) { return PLANAR(Map, block, map_dev); }

int lumahip_moments_map_dims(unsigned w, unsigned h, unsigned block, unsigned *nbx, unsigned *nby) { return map_dims(DistWhat::Moments, w, h, block, nbx, nby); }
int lumahip_moments_map_frames_device(lumahip_ctx *c, const float *rgb, MEASURE_PARAMS, unsigned block, uint64_t *mom_dev) { return PACKED(Moments, block, mom_dev); }
int lumahip_moments_map_frames_device_planar(lumahip_ctx *c, const float *const rgb_planes[3], MEASURE_PARAMS, unsigned block, uint64_t *mom_dev) { return PLANAR(Moments, block, mom_dev); }
int lumahip_moments_map_frames_device_f16(lumahip_ctx *c, const uint16_t *rgb, MEASURE_PARAMS, unsigned block, uint64_t *mom_dev) { return PACKED(Moments, block, mom_dev); }
int lumahip_moments_map_frames_device_planar_f16(lumahip_ctx *c, const uint16_t *const rgb_planes[3], MEASURE_PARAMS, unsigned block, uint64_t *mom_dev) { return PLANAR(Moments, block, mom_dev); }
}  // extern "C"
