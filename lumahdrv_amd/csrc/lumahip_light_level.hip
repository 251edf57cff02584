// lumahip_light_level.hip -- the content light level calls (include/lumahip_compare.h): per frame the eight integer words MaxCLL and
// MaxFALL are made of, over max(R, G, B) and over the luminance, of frames as they are (lh::k_light_level, luma_kernels.hpp: float or
// binary16, no quantizer, no tables, no dynamic LDS) or of code planes under the context's quantizer (lh::k_planes_light_level: the
// floats lumahip_decode_frames_device would write, never written).  The twenty kernels are named here and nowhere else; beside them
// the two pickers, the plan of a launch (light_plan, on lumahip_internal.hpp's MeasureOut and shared checks), the one dispatch (light_level_impl) and the five _device entry points.  The
// host forms are lumahip_host.hip's.
#include "lumahip_internal.hpp"

using namespace lh;
using namespace lhost;

namespace lhost {

typedef void (*light_kernel_t)(const lh::LightArgs);
typedef void (*planes_light_kernel_t)(const lh::PlanesLightArgs);

static light_kernel_t pick_light(int vw, bool in16)
{
    if (in16)
        return vw == 4 ? k_light_level<4, true> : k_light_level<2, true>;
    return vw == 4 ? k_light_level<4, false> : k_light_level<2, false>;
}

template <int CS>
static planes_light_kernel_t pick_planes_light_cs(bool sub, int vw)
{
    if (sub)
        return vw == 4 ? k_planes_light_level<CS, true, 4> : k_planes_light_level<CS, true, 2>;
    return vw == 4 ? k_planes_light_level<CS, false, 4> : k_planes_light_level<CS, false, 2>;
}

static planes_light_kernel_t pick_planes_light(int cs, bool sub, int vw)
{
    switch (cs) {
    case CS_LUV: return pick_planes_light_cs<CS_LUV>(sub, vw);
    case CS_YCBCR: return pick_planes_light_cs<CS_YCBCR>(sub, vw);
    case CS_RGB: return pick_planes_light_cs<CS_RGB>(sub, vw);
    case CS_XYZ: return pick_planes_light_cs<CS_XYZ>(sub, vw);
    }
    return nullptr;
}

// Workgroups per CU of the plane-fed family where grid_for's rules would have decided: 256-thread workgroups (every colour space but
// YCbCr) / the 512-thread workgroups of YCbCr (light_plan says why).  The frame-fed family keeps the rule's three.
static constexpr int LIGHT_PLANES_PER_CU = 5, LIGHT_PLANES_Y_PER_CU = 3;

// What light_plan decides for a launch: the front end, the kernel's key, the launch shape and the kernel's arguments
struct LightPlan {
    bool planes, in16, sub;
    int cs, vw, threads, grid;
    size_t lds;           // dynamic LDS of the launch (the eight words the waves meet in are static and counted in the budget)
    LightArgs f;          // the frame-fed launch
    PlanesLightArgs p;    // the plane-fed launch
};

// The one place that decides what a light-level launch may be and how it runs; exactly one of `f` (frames) and `pl` (code planes
// under the context's quantizer and sc) is given.  Every error is raised here, before anything of the launch is queued.  The
// frame-fed forms read no quantizer: a context that never had one set is fine.
static int light_plan(lumahip_ctx *c, const SrcFrames *f, const SrcPlanes *pl, float sc, float scale, const MeasureOut &m, uint64_t *out,
                      LightPlan &p)
{
    const unsigned nframes = m.nframes, w = m.w, h = m.h;
    p.planes = pl != nullptr;
    int rc;
    if ((rc = f ? check_plane_sets(c, {}, f->plane[0] && f->plane[1] && f->plane[2]) : check_plane_sets(c, {{*pl}}, true)))
        return rc;
    if (nframes == 0)
        return fail(c, LUMAHIP_ERR_ARG, "light level: nframes must be at least 1");
    if ((rc = check_size(c, w, h)) || (rc = check_light_scale(c, scale)) || (rc = m.check_out(c, out)))
        return rc;
    HIPCHK(c, hipSetDevice(c->device));
    p.f = LightArgs{};
    p.p = PlanesLightArgs{};
    p.lds = 0;
    p.in16 = p.sub = false;
    p.cs = 0;
    FrameGeom *g;
    if (f) {
        p.in16 = f->elem == Elem::F16;
        bool al4;
        // (the words may not share a byte with anything the launch reads)
        if ((rc = check_frame_alignment(c, *f, elem_size(f->elem), &al4)) || (rc = check_out_overlap(c, m, out, f, {})))
            return rc;
        p.vw = al4 ? 4 : 2;
        // no tables: the workgroup is the context's (lumahip_tune "block"), clamped to what the kernels are compiled for
        p.threads = std::min(block_threads_for(c, 0), LIGHT_BOUND);
        for (int k = 0; k < 3; k++)
            p.f.e.src[k] = static_cast<const float *>(f->plane[k]);   // (the IN16 kernels read the same pointers as halves)
        p.f.e.frame_stride = f->frame_stride;
        p.f.scale = scale;
        p.f.out = out;
        g = &p.f.e.g;
    } else {
        const int profile = pl->profile;
        if ((rc = check_profile(c, profile)))
            return rc;
        if (!c->have_quant)
            return fail(c, LUMAHIP_ERR_STATE, "quantizer not set (call lumahip_set_quantizer first)");
        if ((rc = check_planes_layout(c, *pl, nframes, w, h)) || (rc = check_out_overlap(c, m, out, nullptr, {{*pl}})))
            return rc;
        // ---- the supported set: the tables the decode call would stage in LDS; what it leaves in global memory is refused here
        const int cs = c->q.cs;
        if (cs != CS_LUV && cs != CS_YCBCR && cs != CS_RGB && cs != CS_XYZ)
            return fail(c, LUMAHIP_ERR_UNSUPPORTED, "planes light level: no kernel for colour space %d", cs);
        // (the transcode calls' rule for their source side: depths up to 12 bits, whatever lumahip_tune "lds_table_max_kb" would still stage)
        if (c->bitdepth > 12 || c->bitdepthC > 12 || !c->lut_in_lds)
            return fail(c, LUMAHIP_ERR_UNSUPPORTED, "planes light level: the tables must be staged in LDS (bit depths <= 12, got %u / %u)", c->bitdepth,
                        c->bitdepthC);
        if (cs == CS_YCBCR && !c->q.ytab)
            return fail(c, LUMAHIP_ERR_UNSUPPORTED, "planes light level: no y table for this YCbCr stream (table values, LDS size or lumahip_tune \"ycbcr_tables\")");
        p.lds = lds_bytes(c, false, cs);
        if (p.lds + m.lds_bytes() > LUMAHIP_LDS_PER_WORKGROUP)
            return fail(c, LUMAHIP_ERR_UNSUPPORTED, "planes light level: the tables take %zu bytes of LDS, a workgroup has %zu", p.lds, LUMAHIP_LDS_PER_WORKGROUP);
        p.cs = cs;
        p.sub = (profile == 0 || profile == 2);
        // four pixels per thread and row when the width and the planes allow the vector accesses, else two (read byte by byte
        // where the planes do not take them at that width either: DecArgs::aligned)
        p.vw = ((w % 4) == 0 && planes_aligned(*pl, 4)) ? 4 : 2;
        p.threads = std::min(block_threads_for(c, p.lds, false, cs == CS_YCBCR), cs == CS_YCBCR ? LightFront<CS_YCBCR>::bound : LightFront<CS_LUV>::bound);
        p.p.d.q = c->q;
        p.p.d.q.cs = cs;
        p.p.d.sc = sc;
        read_planes(p.p.d, *pl, p.vw);
        p.p.scale = scale;
        p.p.out = out;
        g = &p.p.d.g;
    }
    if (!make_geom(*g, w, h, p.vw, p.threads / 64, nframes))
        return fail(c, LUMAHIP_ERR_ARG, "batch too large: more than 2^31 tiles in one launch");
    // The launch rules start from the encode kernels' (frames: grid_for dir 0, three 256-thread workgroups per CU) and the transcode
    // kernels' (planes: the same with `transcode`; YCbCr: 12 / 18 workgroups of 512 threads).  The in-process interleaved sweep of
    // "blocks_per_cu" over {3, 5, 8} (tools/bench/light_level.py --sweep, profiles/light_level.jsonl; ms per launch of
    // 8 x 4K): float frames 0.159 / 0.183 / 0.177 and binary16 frames 0.135 / 0.165 / 0.161 -- the frame-fed family keeps the rule's 3
    // (its two units in flight per wave are the concurrency; more workgroups are more atomics per frame on the same eight words);
    // PQ-11 Lu'v' planes 0.194 / 0.177 / 0.212 -- 5, as the plane-to-plane maps, whose single-buffered loads only other waves cover;
    // HDR10 planes 0.463 / 0.464 / 0.491 against 0.492 under the rule's 12 -- 3: two 512-thread workgroups are resident per CU, and
    // every further one stages the decode tables anew.  grid_for keeps the precedence of lumahip_tune "blocks_per_cu", "grid_enc" and
    // "lane_grid_enc" over either value.
    const int own = !pl ? 0 : (p.cs == CS_YCBCR && p.threads == 512) ? LIGHT_PLANES_Y_PER_CU : p.threads == 256 ? LIGHT_PLANES_PER_CU : 0;
    p.grid = grid_for(c, p.threads, g->totalTiles, 0, 0, (pl && p.cs == CS_YCBCR) ? 1 : 0, pl != nullptr, own);
    return LUMAHIP_OK;
}

int light_level_impl(lumahip_ctx *c, const SrcFrames *f, const SrcPlanes *pl, float sc, float scale, const MeasureOut &m, uint64_t *out,
                     const StreamLaunch &o)
{
    LightPlan p;
    if (int rc = light_plan(c, f, pl, sc, scale, m, out, p))
        return rc;
    const hipStream_t s = launch_stream(c, o.stream, o.lanes);
    if (!p.planes)
        return launch_measure(c, m, out, pick_light(p.vw, p.in16), p.grid, p.threads, 0, s, p.f);
    const planes_light_kernel_t kern = pick_planes_light(p.cs, p.sub, p.vw);
    if (!kern)
        return fail(c, LUMAHIP_ERR_UNSUPPORTED, "no planes light level kernel for colour space %d", p.cs);
    return launch_measure(c, m, out, kern, p.grid, p.threads, p.lds, s, p.p);
}

// what the four frame-fed _device entry points do in front of the dispatch; frames_given: the packed forms' base pointer (the planar
// forms' three pointers are light_plan's to check)
static int light_frames_entry(lumahip_ctx *c, bool frames_given, const SrcFrames &f, float scale, uint64_t *out)
{
    return device_entry(c, frames_given, [&](const StreamLaunch &o) {
        return light_level_impl(c, &f, nullptr, 1.0f, scale, {DistWhat::Light, "light level", 0, f.nframes, f.w, f.h}, out, o);
    });
}

}  // namespace lhost

// The five _device entry points (include/lumahip_compare.h has their full prototypes and the statistic's text)
#define LIGHT_PARAMS size_t frame_stride, unsigned nframes, unsigned w, unsigned h, float scale, uint64_t *out_dev
#define PACKED light_frames_entry(c, rgb != nullptr, packed_frames(rgb, frame_stride, nframes, w, h), scale, out_dev)
#define PLANAR light_frames_entry(c, true, planar_frames(rgb_planes, frame_stride, nframes, w, h), scale, out_dev)
extern "C" {
int lumahip_light_level_frames_device(lumahip_ctx *c, const float *rgb, LIGHT_PARAMS) { return PACKED; }
int lumahip_light_level_frames_device_planar(lumahip_ctx *c, const float *const rgb_planes[3], LIGHT_PARAMS) { return PLANAR; }
int lumahip_light_level_frames_device_f16(lumahip_ctx *c, const uint16_t *rgb, LIGHT_PARAMS) { return PACKED; }
int lumahip_light_level_frames_device_planar_f16(lumahip_ctx *c, const uint16_t *const rgb_planes[3], LIGHT_PARAMS) { return PLANAR; }

int lumahip_planes_light_level_frames_device(lumahip_ctx *c, const unsigned char *const planes[3], const int stride[3], const size_t pfs[3],
                                             unsigned nframes, unsigned w, unsigned h, int profile, float sc, float scale, uint64_t *out_dev)
{
    const SrcPlanes pl{planes, stride, pfs, profile};
    return device_entry(c, true, [&](const StreamLaunch &o) {
        return light_level_impl(c, nullptr, &pl, sc, scale, {DistWhat::Light, "light level", 0, nframes, w, h}, out_dev, o);
    });
}
}  // extern "C"
