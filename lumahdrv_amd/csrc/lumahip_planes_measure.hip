// lumahip_planes_measure.hip -- the plane-to-plane measuring calls (include/lumahip_compare.h): how far apart two sets of code planes
// are, as integer sums per frame and plane (lh::k_planes_distortion, luma_kernels.hpp), per block (k_planes_distortion_map) or as the
// moments of both signals per block (k_planes_moments_map).  e and g are the samples present in the two sets: no quantizer, no tables,
// no dynamic LDS.  The twelve kernels are named here and nowhere else; beside them the picker, the plan of a launch (planes_plan: vector width, workgroup
// and grid; what the launch delivers and the checks are lumahip_internal.hpp's MeasureOut and shared checks), the one dispatch
// (planes_measure_impl) and the three _device entry points.  The host forms are lumahip_host.hip's.
#include "lumahip_internal.hpp"

using namespace lh;
using namespace lhost;

namespace lhost {

typedef void (*planes_kernel_t)(const lh::PlanesMeasureArgs);

template <bool SUB, int VW>
static planes_kernel_t pick_planes_measure_what(DistWhat what)
{
    switch (what) {
    case DistWhat::Frame: return k_planes_distortion<SUB, VW>;
    case DistWhat::Map: return k_planes_distortion_map<SUB, VW>;
    case DistWhat::Moments: return k_planes_moments_map<SUB, VW>;
    case DistWhat::Light: break;   // (lumahip_light_level.hip's)
    }
    return nullptr;
}

static planes_kernel_t pick_planes_measure(DistWhat what, bool sub, int vw)
{
    if (sub)
        return vw == 4 ? pick_planes_measure_what<true, 4>(what) : pick_planes_measure_what<true, 2>(what);
    return vw == 4 ? pick_planes_measure_what<false, 4>(what) : pick_planes_measure_what<false, 2>(what);
}

static constexpr int PLANES_MAP_PER_CU = 5;   // 256-thread workgroups per CU of the two map launches (planes_plan says why)

// What planes_plan decides for a launch over two plane sets as they are: vector width, launch shape and the kernel's arguments
struct PlanesPlan {
    bool sub;
    int vw, threads, grid;
    PlanesMeasureArgs k;
};

// The one place that decides what such a launch may be and how it runs.  Every error is raised here, the block size first, before
// anything of the launch is queued.  Reads no quantizer: a context that never had one set is fine.
static int planes_plan(lumahip_ctx *c, const SrcPlanes &a, const SrcPlanes &b, const MeasureOut &m, uint64_t *out, PlanesPlan &p)
{
    const bool map = m.map();
    const unsigned nframes = m.nframes, w = m.w, h = m.h;
    const int profile = b.profile;
    int rc;
    if ((rc = m.check_block(c)) || (rc = check_plane_sets(c, {{a}, {b}}, nframes != 0)) || (rc = check_size(c, w, h)) ||
        (rc = check_profile(c, profile)) || (rc = check_planes_layout(c, a, nframes, w, h)) || (rc = check_planes_layout(c, b, nframes, w, h)) ||
        // both plane sets are read only and may overlap each other; the words may not share a byte with anything the launch reads
        (rc = m.check_out(c, out)) || (rc = check_out_overlap(c, m, out, nullptr, {{a, "", " of set A"}, {b, "", " of set B"}})))
        return rc;
    HIPCHK(c, hipSetDevice(c->device));

    p.sub = (profile == 0 || profile == 2);
    // four pixels per thread and row when the width and at least one set allow the vector accesses, else two; a set that does not
    // take them at the chosen width is read byte by byte (DecArgs::aligned, per set, as read_planes decides for given planes)
    p.vw = ((w % 4) == 0 && (planes_aligned(a, 4) || planes_aligned(b, 4))) ? 4 : 2;
    // no tables: the workgroup is the context's (lumahip_tune "block"), clamped to what the kernels are compiled for and, for the
    // maps, by the record's rule
    p.threads = m.clamp_threads(std::min(block_threads_for(c, 0), PLANES_MEASURE_BOUND));
    p.k = PlanesMeasureArgs{};
    if (!make_geom(p.k.a.g, w, h, p.vw, p.threads / 64, nframes))
        return fail(c, LUMAHIP_ERR_ARG, "batch too large: more than 2^31 tiles in one launch");
    p.k.g.g = p.k.a.g;
    read_planes(p.k.a, a, p.vw);
    read_planes(p.k.g, b, p.vw);
    p.k.out = out;
    // The launch rule starts from three 256-thread workgroups per CU, the rule of the other plane-fed measuring calls -- which is what
    // grid_for gives a 256-thread launch of direction 0 without YCbCr -- and the per-frame words keep it.  The two maps take
    // PLANES_MAP_PER_CU: the sweep of "blocks_per_cu" over {3, 5, 8} (profiles/planes_measure.jsonl) has the per-frame
    // words fastest at 3 -- more workgroups are more atomics per frame on the same 12 words -- and the maps at 5: a map launch has no
    // arithmetic to hide its loads behind, only other waves.  grid_for keeps the precedence of lumahip_tune "blocks_per_cu",
    // "grid_enc" and "lane_grid_enc" over either value.
    p.grid = grid_for(c, p.threads, p.k.a.g.totalTiles, 0, 0, 0, false, (map && p.threads == 256) ? PLANES_MAP_PER_CU : 0);
    map_shape(m, p.k.a.g, p.threads, p.k.m, p.grid);
    return LUMAHIP_OK;
}

int planes_measure_impl(lumahip_ctx *c, const SrcPlanes &a, const SrcPlanes &b, const MeasureOut &m, uint64_t *out, const StreamLaunch &o)
{
    PlanesPlan p;
    if (int rc = planes_plan(c, a, b, m, out, p))
        return rc;
    const planes_kernel_t kern = pick_planes_measure(m.kind, p.sub, p.vw);
    if (!kern)
        return fail(c, LUMAHIP_ERR_UNSUPPORTED, "no planes measuring kernel");
    return launch_measure(c, m, out, kern, p.grid, p.threads, 0, launch_stream(c, o.stream, o.lanes), p.k);
}

}  // namespace lhost

// The three _device entry points (include/lumahip_compare.h has their full prototypes): PLANES_PARAMS, then the call's own tail.
#define PLANES_PARAMS                                                                                                                       \
    const unsigned char *const a_planes[3], const int a_stride[3], const size_t a_pfs[3], unsigned nframes, unsigned w, unsigned h,           \
        const unsigned char *const b_planes[3], const int b_stride[3], const size_t b_pfs[3], int profile
#define CALL_Frame "planes distortion"
#define CALL_Map "planes distortion map"
#define CALL_Moments "planes moments map"
#define PLANES(what, block, out)                                                                                                            \
    device_entry(c, true, [&](const StreamLaunch &o) {                                                                                      \
        return planes_measure_impl(c, {a_planes, a_stride, a_pfs, profile}, {b_planes, b_stride, b_pfs, profile},                           \
                                   {DistWhat::what, CALL_##what, block, nframes, w, h}, out, o);                                            \
    })
extern "C" {
int lumahip_planes_distortion_frames_device(lumahip_ctx *c, PLANES_PARAMS, uint64_t *out_dev) { return PLANES(Frame, 0, out_dev); }
int lumahip_planes_distortion_map_frames_device(lumahip_ctx *c, PLANES_PARAMS, unsigned block, uint64_t *map_dev) { return PLANES(Map, block, map_dev); }
int lumahip_planes_moments_map_frames_device(lumahip_ctx *c, PLANES_PARAMS, unsigned block, uint64_t *mom_dev) { return PLANES(Moments, block, mom_dev); }
}  // extern "C"
