// lumahip_planes_measure.hip -- the plane-to-plane measuring calls (include/lumahip_compare.h): how far apart two sets of code planes
// are, as integer sums per frame and plane (lh::k_planes_distortion, luma_kernels.hpp), per block (k_planes_distortion_map) or as the
// moments of both signals per block (k_planes_moments_map).  e and g are the samples present in the two sets: no quantizer, no tables,
// no dynamic LDS.  The twelve kernels are named here and nowhere else; beside them the picker, the plan of a launch (planes_plan), the
// one dispatch (planes_measure_impl) and the three _device entry points.  The host forms are lumahip_host.hip's.
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
static int planes_plan(lumahip_ctx *c, const SrcPlanes &a, unsigned nframes, unsigned w, unsigned h, const SrcPlanes &b, DistWhat kind,
                       unsigned map_block, uint64_t *out, PlanesPlan &p)
{
    const bool map = kind != DistWhat::Frame, moments = kind == DistWhat::Moments;
    const char *const what = moments ? "planes moments map" : map ? "planes distortion map" : "planes distortion";
    const char *const out_name = moments ? "mom_dev" : map ? "map_dev" : "out_dev";
    if (map && !dist_block_ok(kind, map_block))
        return fail(c, LUMAHIP_ERR_ARG, "%s: block must be %s16, 32 or 64 (got %u)", what, moments ? "8, " : "", map_block);
    if (!a.planes || !a.stride || !a.pfs || !b.planes || !b.stride || !b.pfs || nframes == 0)
        return fail(c, LUMAHIP_ERR_ARG, "null argument");
    for (int k = 0; k < 3; k++)
        if (!a.planes[k] || !b.planes[k])
            return fail(c, LUMAHIP_ERR_ARG, "null plane %d", k);
    // (check_geom's tests without its demand for a quantizer)
    if (w == 0 || h == 0 || (w & 1) || (h & 1))
        return fail(c, LUMAHIP_ERR_ARG, "Invalid frame size %ux%u (must be even, non-zero)", w, h);
    const int profile = b.profile;
    if (profile < 0 || profile > 3 || a.profile != profile)
        return fail(c, LUMAHIP_ERR_ARG, "profile must be 0..3 (got %d)", profile);
    const SrcFrames geom{{nullptr, nullptr, nullptr}, Elem::F32, 0, nframes, w, h};   // (the code planes' checks read the geometry only)
    int rc;
    if ((rc = check_layout(c, geom, false, a.stride, a.pfs, profile)) || (rc = check_layout(c, geom, false, b.stride, b.pfs, profile)))
        return rc;
    // both plane sets are read only and may overlap each other; the words may not share a byte with anything the launch reads
    if (map) {
        if (!out || !is_aligned(out, 8))
            return fail(c, LUMAHIP_ERR_ARG, "%s must be non-null and 8-byte aligned", out_name);
    } else if ((rc = check_out_words(c, out))) {
        return rc;
    }
    const size_t out_bytes =
        map ? (size_t)nframes * dist_map_words(w, h, map_block, dist_words_per_block(kind)) * sizeof(uint64_t) : out_words_bytes(nframes);
    for (int k = 0; k < 3; k++) {
        if (out_overlaps_plane(out, out_bytes, a, k, w, h, nframes))
            return fail(c, LUMAHIP_ERR_ARG, "%s overlaps plane %d of set A", out_name, k);
        if (out_overlaps_plane(out, out_bytes, b, k, w, h, nframes))
            return fail(c, LUMAHIP_ERR_ARG, "%s overlaps plane %d of set B", out_name, k);
    }
    HIPCHK(c, hipSetDevice(c->device));

    p.sub = (profile == 0 || profile == 2);
    // four pixels per thread and row when the width and at least one set allow the vector accesses, else two; a set that does not
    // take them at the chosen width is read byte by byte (DecArgs::aligned, per set, as read_planes decides for given planes)
    p.vw = ((w % 4) == 0 && (planes_aligned(a, 4) || planes_aligned(b, 4))) ? 4 : 2;
    // no tables: the workgroup is the context's (lumahip_tune "block"), clamped to what the kernels are compiled for and, for the
    // maps, to the 2 NW rows of a standard tile dividing the block (every workgroup size is a power of two)
    p.threads = std::min(block_threads_for(c, 0), PLANES_MEASURE_BOUND);
    if (map)
        p.threads = std::min(p.threads, 32 * (int)map_block);
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
    if (map) {
        // a workgroup takes whole map tiles
        p.k.m = make_map_geom(p.k.a.g, w, h, map_block, p.threads);
        p.grid = std::min(p.grid, p.k.m.totalMapTiles);
    }
    return LUMAHIP_OK;
}

int planes_measure_impl(lumahip_ctx *c, const SrcPlanes &a, unsigned nframes, unsigned w, unsigned h, const SrcPlanes &b, DistWhat what,
                        unsigned block, uint64_t *out, const PlanesLaunch &o)
{
    PlanesPlan p;
    if (int rc = planes_plan(c, a, nframes, w, h, b, what, block, out, p))
        return rc;
    const planes_kernel_t kern = pick_planes_measure(what, p.sub, p.vw);
    if (!kern)
        return fail(c, LUMAHIP_ERR_UNSUPPORTED, "no planes measuring kernel");
    const hipStream_t s = launch_stream(c, o.stream, o.lanes);
    if (what == DistWhat::Frame)
        return launch_measuring(c, kern, p.grid, p.threads, 0, s, p.k, nframes);
    if (int rc = launch_fused(c, kern, p.grid, p.threads, 0, s, p.k))
        return rc;
    HIPCHK(c, hipGetLastError());
    return LUMAHIP_OK;
}

// what the three _device entry points do in front of the dispatch
static int planes_measure_entry(lumahip_ctx *c, const SrcPlanes &a, unsigned nframes, unsigned w, unsigned h, const SrcPlanes &b, DistWhat what,
                                unsigned block, uint64_t *out)
{
    if (!c)
        return LUMAHIP_ERR_ARG;
    return planes_measure_impl(c, a, nframes, w, h, b, what, block, out, {c->stream, true});
}

}  // namespace lhost

// The three _device entry points (include/lumahip_compare.h has their full prototypes): PLANES_PARAMS, then the call's own tail.
#define PLANES_PARAMS                                                                                                                       \
    const unsigned char *const a_planes[3], const int a_stride[3], const size_t a_pfs[3], unsigned nframes, unsigned w, unsigned h,           \
        const unsigned char *const b_planes[3], const int b_stride[3], const size_t b_pfs[3], int profile
#define PLANES(what, block, out) \
    planes_measure_entry(c, {a_planes, a_stride, a_pfs, profile}, nframes, w, h, {b_planes, b_stride, b_pfs, profile}, DistWhat::what, block, out)
extern "C" {
int lumahip_planes_distortion_frames_device(lumahip_ctx *c, PLANES_PARAMS, uint64_t *out_dev) { return PLANES(Frame, 0, out_dev); }
int lumahip_planes_distortion_map_frames_device(lumahip_ctx *c, PLANES_PARAMS, unsigned block, uint64_t *map_dev) { return PLANES(Map, block, map_dev); }
int lumahip_planes_moments_map_frames_device(lumahip_ctx *c, PLANES_PARAMS, unsigned block, uint64_t *mom_dev) { return PLANES(Moments, block, mom_dev); }
}  // extern "C"
