// lumahip_internal.hpp -- what the translation units behind include/lumahip.h share: the context, error helpers,
// launch-geometry rules and the device-side implementations the host entry points call.  Not installed, not part of the ABI.
//
//   lumahip_core.hip    context life cycle, the per-stream tables of a quantizer (which, when, how large), layout checks,
//                       memory helpers                                                                    (no kernels)
//   lumahip_tables.hpp  what those tables are made of: owning device buffer, process-wide host cache, per-context LRU
//   lumahip_launch.hip  launch geometry: LDS bytes, threads per workgroup, persistent workgroups per CU   (no kernels)
//   lumahip_pick.hpp    which instantiation of the fused kernels a launch takes: pick_enc<IN16> / pick_dec<OUT16> / pick_dist<IN16> /
//                       pick_planes<TransFamily | TransHalfFamily | TransQuarterFamily | TransDistFamily | TransDistMapFamily | TransMomentsMapFamily |
//                       TransHalfDistFamily | TransHalfDistMapFamily, VW>, included by the kernel units below and by nothing else
//   lumahip_encode.hip  pick_enc<false> (every float-frame k_encode), the encode dispatch, the other encode-side kernels
//   lumahip_decode.hip  pick_dec<false> (every float-frame k_decode), the decode dispatch, the array kernels, the red / blue
//                       tables next to the kernel that builds them
//   lumahip_encode_f16.hip / lumahip_decode_f16.hip  pick_enc<true> / pick_dec<true> (the binary16-frame kernels, exported as
//                       pick_enc_f16 / pick_dec_f16 to the two dispatch functions) and the _f16 device entry points (+ the
//                       narrowing probe)
//   lumahip_transcode.hip  pick_planes<TransFamily, .> (every k_transcode), transcode_plan -- what a launch over two plane sets may
//                       be --, the transcode dispatch and its entry point; measure_planes_impl, the one dispatch of the five plane-fed
//                       measuring calls, and their five _device entry points (two of them include/lumahip_ladder.h's)
//   lumahip_transcode_half.hip  pick_planes<TransHalfFamily, .> (every k_transcode_half), the half-resolution transcode's dispatch
//                       (transcode_plan with scale 2) and its _device entry point of include/lumahip_compare.h
//   lumahip_transcode_quarter.hip  pick_planes<TransQuarterFamily, .> (every k_transcode_quarter), the quarter-resolution transcode's
//                       dispatch (transcode_plan with scale 4) and its _device entry point of include/lumahip_rungs.h
//   lumahip_transcode_distortion.hip / lumahip_transcode_distortion_map.hip / lumahip_transcode_moments_map.hip  pick_planes<
//                       TransDistFamily | TransDistMapFamily | TransMomentsMapFamily, .> (every k_transcode_distortion /
//                       k_transcode_distortion_map / k_transcode_moments_map), exported as pick_transdist / pick_transdist_map /
//                       pick_transdist_moments_map; nothing else
//   lumahip_transcode_half_distortion.hip / lumahip_transcode_half_distortion_map.hip  pick_planes<TransHalfDistFamily |
//                       TransHalfDistMapFamily, .> (every k_transcode_half_distortion / k_transcode_half_distortion_map), exported as
//                       pick_transhalf_dist / pick_transhalf_dist_map; nothing else
//   lumahip_distortion.hip  pick_dist<DistFamily, false> (every float-frame k_distortion), distortion_plan -- what a launch that scores
//                       given planes against frames may be --, measure_frames_impl, the one dispatch of the frame-fed measuring calls
//                       (distortion, distortion map, moments map), their twelve _device entry points and the two *_map_dims
//   lumahip_distortion_f16.hip, lumahip_distortion_map.hip / _f16.hip, lumahip_moments_map.hip / _f16.hip  pick_dist<DistFamily, true>,
//                       pick_dist<DistMapFamily, .>, pick_dist<MomentsMapFamily, .> (the other frame-fed measuring kernels), exported
//                       as pick_dist_f16, pick_dist_map_f32 / _f16, pick_moments_map_f32 / _f16; nothing else
//   lumahip_planes_measure.hip  the twelve k_planes_distortion / k_planes_distortion_map / k_planes_moments_map kernels (two plane sets
//                       as they are, no quantizer), their picker, planes_plan, the dispatch planes_measure_impl and the three
//                       _device entry points of include/lumahip_compare.h
//   lumahip_light_level.hip  the twenty k_light_level / k_planes_light_level kernels (content light level of frames as they are and of
//                       code planes under the context's quantizer), their pickers, light_plan, the dispatch light_level_impl and the
//                       five _device entry points of include/lumahip_compare.h
//   The four plans of the measuring calls (transcode_plan, distortion_plan, planes_plan, light_plan) keep what is a family's own:
//   the quantizers it needs, its supported set and LDS budget, vector width, the workgroup bound and grid_for's arguments.  What a
//   launch delivers -- words, the output's name in messages, valid blocks, LDS to meet in, zeroed or not -- is one record, MeasureOut,
//   below; the checks of the plane sets, the size, the layout, the output pointer and its overlaps, the map's shape (map_shape), the
//   closing launch (launch_measure), the launch options (StreamLaunch) and the entry helper (device_entry) stand beside it, once.
//   lumahip_misc.hip    stand-alone transform, synthetic frames, the reference's mean luminance, probes, timing helper
//   lumahip_host.hip    the _host entry points: staging, host <-> device transfers, the one 3-stage pipeline of the banded,
//                       batched and stream push / pop forms, the one host form of the thirteen measuring calls (measure_host)
//                                                                                                         (no kernels)
//   lumahip_pool.hip    the HBM chunk pool;  lumahip_multi.hip  many GPUs in one process                  (no kernels)
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#define LUMAHIP_EXPERIMENTAL   /* the library defines what the experimental section of the header declares */
#include "../../include/lumahip.h"
#include "../../include/lumahip_measure.h"
#include "../../include/lumahip_compare.h"
#include "../../include/lumahip_ladder.h"
#include "../../include/lumahip_rungs.h"
#include "luma_kernels.hpp"
#include "host_lut.hpp"
#include "lut_index.hpp"
#include "numa_host.hpp"
#include "lumahip_tables.hpp"

// Largest search table (encode: threshold records, decode: the luminance table) a workgroup stages in LDS; beyond it
// the table is read from global memory (L2-resident).  gfx950 has 160 KiB of LDS per CU; tables beyond 53 KiB run as one
// or two 1024-thread workgroups per CU -- for the 136 KiB of PQ 13-bit records that is still twice as fast as gathering
// them from L2 (346 against 182 Gpixel/s, profiles/r02_perf_matrix.txt).  LUMAHIP_LDS_TABLE_MAX_KB overrides it.
static constexpr size_t LUMAHIP_LDS_TABLE_MAX_DEFAULT = 144 * 1024;
static constexpr size_t LUMAHIP_LDS_PER_WORKGROUP = 160 * 1024;
static constexpr int LUMAHIP_MAX_LANES = 4;

// Kernel choice from feedback, as a function of the data and of nothing else (lumahip_core.hip lag_policy_*).  Two pairs of
// kernels compute the same results at different speeds depending on what the stream holds: the YCbCr encode kernels with the
// half-input table (fast on binary16-valued frames, 1.4 x slower than the per-pixel kernels on others) and the YCbCr decode
// kernels that may read red / blue from the per-stream tables (fast on pictures, a few per cent slower than the plain ones on
// unrelated pixels, where no wave ever takes the tables).  Every launch of the data-dependent ("fast") kernel gets its OWN word
// in a ring of pinned host memory, which the kernel sets to 1 as documented at EncArgs::half_flag / DecArgs::rb_flag, and an
// event recorded behind it; the host reads launch j's word when it issues the eligible launch LAG later, after that event has
// completed (normally long ago; at most LAG - 1 launches stay queued behind it, so the device does not run dry).  States:
//   ON_FAST     fast launches; a BAD word -> BACKOFF for 16 launches (the words of the other launches in flight are dropped);
//   BACKOFF     plain launches; when the count runs out, ONE fast launch probes -> PROBE_WAIT;
//   PROBE_WAIT  plain launches until the probe's word is read (LAG launches later): bad -> BACKOFF with the pause doubled (up
//               to max_backoff), good -> ON_FAST and the pause forgotten.
// max_backoff weighs a probe's cost against a missed switch: a half-table probe on float data costs 40 % of its launch (1024:
// 0.04 % of the stream), a red / blue probe on unrelated pixels 3 % while a picture decoded without the tables loses a third (64).
// `report_is_bad`: whether a set word (true) or a clear one (false) is the bad news.
struct LagPolicy {
    static constexpr int LAG = 4, RING = 8;
    enum { ON_FAST = 0, BACKOFF = 1, PROBE_WAIT = 2 };
    LagPolicy(bool bad_when_set, int longest_pause) : report_is_bad(bad_when_set), max_backoff(longest_pause) {}
    bool report_is_bad;
    int max_backoff;                                 // the pause doubles from 16 up to this many launches
    uint32_t *h_flag = nullptr;                      // RING words of pinned host memory
    hipEvent_t ev[RING] = {};
    struct Pending {
        unsigned long issued_at;                     // index of the eligible launch this fast launch was
        int slot;
        bool probe;                                  // the single fast launch at the end of a back-off
    };
    std::vector<Pending> pending;                    // oldest first; at most LAG entries
    unsigned long elig = 0;                          // eligible launches so far (fast or not)
    unsigned long seq = 0;                           // fast launches that were given a word
    int state = ON_FAST;
    int backoff = 0, backoff_len = 0;                // plain launches left; length of the current back-off
    unsigned long backoff_launches = 0, bad_words = 0;
};

struct lumahip_copy_pool;                                   // lumahip_host.hip: worker threads of the staging copies
void lumahip_copy_pool_destroy(lumahip_copy_pool *p);

struct lumahip_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    std::string err;
    int num_cu = 256;

    bool have_quant = false;
    int ptf = 0;
    unsigned bitdepth = 0, bitdepthC = 0;
    lh::QuantDev q{};
    // The device tables of the quantizer (lumahip_core.hip upload_table / ensure_search_index publish them in q and q_y): the
    // luminance table and, YCbCr only, the per-stream y table of the decode kernels (host_lut.cpp); the encode-side search
    // records (float-bit or value-keyed, built on first use) and, YCbCr only, those of the composite luma -> code function
    lhost::DevTable<float> d_lut, d_ytab;
    lhost::DevTable<uint32_t> d_rec, d_rec_y;
    std::shared_ptr<const lh::ThreshIndex> tix;  // what d_rec was uploaded from, unless the records are value-keyed (lumahip_quantizer_info)
    bool use_lin_index = true;                   // lumahip_tune("lin_index", 0): no value-keyed records (A/B, tests)
    bool index_ready = false;
    lh::QuantDev q_y{};           // q with the composite records in place of the luminance records
    bool use_ycbcr_tables = true; // lumahip_tune("ycbcr_tables", 0): per-pixel PQ evaluation as in round 2 (A/B, tests)
    // YCbCr encode, binary16 inputs: device copies of the half-input table (luma_device.hpp half_lookup), one per (sc, Lmax) seen;
    // an empty entry records "not usable for this pair" (host_lut.cpp ycbcr_half_table_host).  lumahip_core.hip half_table_for
    struct ScLmax {
        float sc, Lmax;
    };
    lhost::DevTableLru<ScLmax, float, 4> half_tabs;
    int half_mode = 1;            // lumahip_tune("half_table"): 0 = never, 1 = while the stream looks like binary16 data (half_pol: LagPolicy), 2 = always
    LagPolicy half_pol{true, 1024};     // which kernel an eligible YCbCr encode launch takes (half_mode 1): a report = "these are not halves"
    unsigned long half_launches = 0;
    // YCbCr decode: device copies of the per-stream red / blue tables (lumahip_decode.hip rb_table_for), one per preScaling seen
    lhost::DevTableLru<float, float, 2> rb_tabs;
    unsigned long rb_launches = 0;
    bool test_fail_rb_alloc = false;
    bool rb_unavailable = false;  // allocating or building the tables failed for this stream: plain kernels, no retry per launch
    LagPolicy rb_pol{false, 64};      // which kernel an eligible YCbCr decode launch takes (rb_mode 1): NO report = "no wave found its codes local"
    int rb_mode = 1;              // lumahip_tune("ycbcr_rb_tables"): 0 = six powf per pixel (rounds 3-4), 1 = red / blue from the tables where a
                                  // wave's codes are close to each other (luma_kernels.hpp rb_wave_near), 2 = from the tables always
    int dec_vw = 0;               // lumahip_tune("dec_vw", 2): the decode kernels with two pixels per thread and row (0: four where alignment allows)
    int rb_near_y = 64, rb_near_c = 24;    // lumahip_tune("rb_near_y" / "rb_near_c"): the closeness bounds of mode 1 (luma_kernels.hpp rb_wave_local)
    bool force_literal = false;   // lumahip_tune("force_literal"): the reference's bisection instead of the records
    std::vector<float> h_lut;     // host copy of the table handed to lumahip_set_quantizer
    bool lut_in_lds = true;  // decode side: tables up to 12 bits are staged in LDS
    float minLum = 0.0f;

    // The SOURCE quantizer of the transcode calls (lumahip_set_source_quantizer, lumahip_transcode.hip): held beside the quantizer
    // above and independent of it -- setting one never disturbs the other.  Decode-side tables only: the luminance table, the
    // YCbCr y table; the u'v' / chroma-term tables are computed by the kernel as it stages.  No search records, no red / blue
    // tables, no LagPolicy: a transcode launch is chosen from its arguments alone.
    struct SourceQuant {
        bool have = false;
        unsigned bitdepth = 0, bitdepthC = 0;
        lh::QuantDev q{};
        lhost::DevTable<float> d_lut, d_ytab;
        bool lut_in_lds = false;
    } src;

    // staging for the _host entry points
    float *d_frame = nullptr;
    size_t d_frame_cap = 0;
    unsigned char *d_planes = nullptr;
    size_t d_planes_cap = 0;
    float *d_stats = nullptr;
    float *d_stats_part = nullptr;   // partial statistics triples of the encode kernels (STATS_SLOTS per frame)
    size_t d_stats_part_cap = 0;
    float *d_arr = nullptr;
    size_t d_arr_cap = 0;

    // the three device slots of the batched host entry points and of the stream push / pop, and the pipeline's three streams
    // (H2D / kernel / D2H; lumahip_host.hip pipe_run)
    struct Slot {
        float *d_frame = nullptr;
        unsigned char *d_planes = nullptr;
        float *d_stats = nullptr;
        hipEvent_t h2d = nullptr, kern = nullptr, d2h = nullptr;
    } slot[3];
    size_t slot_frame_cap = 0, slot_planes_cap = 0;
    hipStream_t s_h2d = nullptr, s_kern = nullptr, s_d2h = nullptr;
    float *h_stats = nullptr;  // pinned, 3 floats per frame
    // row bands of the single-frame host entry points (H2D of band k+1 | kernel of band k | D2H of band k-1)
    static constexpr int MAX_BANDS = 8;
    hipEvent_t band_h2d[MAX_BANDS] = {}, band_kern[MAX_BANDS] = {};
    float *d_band_stats = nullptr;  // 3 floats per band
    int host_bands = 4;             // lumahip_tune("host_bands"): 1 = the whole frame in one piece
    int band_taper = 70;            // lumahip_tune("band_taper"): each band's rows in % of the previous band's (100 = uniform)
    int up_ramp = 0;                // staged uploads: how many of the small leading chunks of this call have been used
    size_t h_stats_cap = 0;

    // Pinned staging for pageable caller memory (see xfer_h2d): a ring of chunks per direction, N_STAGE up and N_STAGE_DN down
    struct Stage {
        unsigned char *h = nullptr;
        hipEvent_t ev = nullptr;
        bool pending = false;  // a DMA that reads / writes this chunk may still be in flight
        // device -> host only: what to do with the chunk once its DMA has landed (copy it out to the caller's pageable memory)
        unsigned char *out = nullptr;
        size_t out_pitch = 0, chunk_pitch = 0, width = 0, rows = 0;
        unsigned tag = 0;      // which pushed frame the chunk belongs to (lumahip_encode_stream_push); 0 outside a stream
    };
    static constexpr int N_STAGE = 4;   // upload chunks: up to four DMAs queued while the CPU fills the next
    static constexpr int N_STAGE_DN = 8;  // download chunks: a 4K frame's planes are five of them
    Stage stage_up[N_STAGE], stage_dn[N_STAGE_DN];
    unsigned up_next = 0, dn_next = 0;  // ring positions
    size_t dn_chunk = (size_t)8 << 20;  // bytes per download chunk (grows with the frames of the pipelined encode paths)
    // frames pushed with lumahip_encode_stream_push and not yet popped: sequence numbers [es_tail, es_head), frame j in slot[j % 3]
    unsigned es_head = 0, es_tail = 0;
    int es_dir = 0;                // 0: the frames in flight were pushed by lumahip_encode_stream_push, 1: by lumahip_decode_stream_push
    unsigned es_w = 0, es_h = 0;
    int es_profile = 0;
    float es_sc = 1.0f;
    int es_stride[3] = {0, 0, 0};  // plane strides of the frames in flight (a push with other strides is refused)
    float *h_es_stats = nullptr;   // pinned, 3 floats per slot
    unsigned d2h_tag = 0;          // tag given to download chunks queued now
    float *h_small = nullptr;  // pinned scratch for the few-float readbacks
    lumahip_copy_pool *copy_pool = nullptr;
    // NUMA placement of the host side (numa_host.cpp; lumahip_core.hip numa_resolve): the node of this context's GPU and that
    // node's CPUs.  The pinned staging rings are allocated on the node and the copy threads are pinned to its CPUs.
    // lumahip_tune("numa", v): 0 = no placement, as before round 4; 2 (default) = the rings on the GPU's node, the threads left
    // to the scheduler; 1 = rings and threads; 3 = threads only.  Why not 1 by default: on the shared hosts of the GPU boxes
    // (load average 16-33) pinned copy threads cannot move away from cores other tenants keep busy, and the one-frame and
    // pipelined facade calls then dip by up to 30 % every few runs (profiles/r04_numa.txt, second table)
    int numa_mode = 2;
    int numa_force_node = -1;  // lumahip_tune("numa_node", N): pretend the GPU sits on node N (A/B measurements: local against remote)
    bool numa_resolved = false;
    int numa_node = -1;        // -1: not a NUMA box / unknown / switched off
    std::vector<int> numa_cpus;
    // Half upload of the host encode entry points (lumahip_host.hip xfer_h2d_f16): host frames that hold binary16 values cross
    // PCIe as halves.  lumahip_tune("half_upload", v): 0 never, 1 (default) while the frames do hold halves, 2 always try.
    int in16_mode = 1;
    int in16_backoff = 0, in16_backoff_len = 0;
    unsigned long in16_frames = 0, in16_fallbacks = 0;   // frames (or row bands) uploaded as halves / found to hold other values
    bool slot_in16[3] = {false, false, false};           // stream push / pop: what the slot's device frame holds
    int copy_threads = 5;      // lumahip_tune("copy_threads"): worker threads of the staging copies (0 = caller only); 3 until the half
                               // upload, whose conversion is worth two more (batched half-valued 4K frames 4.9 -> 5.6 Gpixel/s; floats: no change)
    int copy_spin = 2000;      // lumahip_tune("copy_spin"): polls of an idle worker before it sleeps

    int block_threads = 256;
    bool block_forced = false;
    bool allow_alias = false;  // LUMAHIP_ALLOW_ALIASED_FRAMES=1: measurement tools alias all frames of a batch onto one
    int blocks_per_cu = 0;  // 0 = occupancy query
    long grid_override[2] = {0, 0};
    size_t lds_table_max = LUMAHIP_LDS_TABLE_MAX_DEFAULT;
    // Unordered sections (lumahip_begin_unordered): successive _device encode / decode calls go round-robin to `lanes_active`
    // internal streams, so that one batch's ramp-up and tail overlap its neighbours' steady state
    hipStream_t lane_stream[LUMAHIP_MAX_LANES] = {};
    hipEvent_t lane_done[LUMAHIP_MAX_LANES] = {};
    hipEvent_t lane_fork = nullptr;
    int lanes_active = 0;
    unsigned lane_next = 0;
    long lane_grid[2] = {0, 0};   // lumahip_tune("lane_grid_enc" / "lane_grid_dec"): workgroups per launch inside a section
    int lanes_default = 0;        // lumahip_tune("lanes"): lanes an unordered section opens with when asked for 0
};

int lumahip_fail(lumahip_ctx *c, int code, const char *fmt, ...) __attribute__((format(printf, 3, 4)));
#define fail lumahip_fail

#define HIPCHK(c, expr)                                                                                        \
    do {                                                                                                       \
        hipError_t e_ = (expr);                                                                                \
        if (e_ != hipSuccess)                                                                                  \
            return fail((c), LUMAHIP_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, \
                        __LINE__);                                                                             \
    } while (0)


namespace lhost {
using namespace lh;

static inline bool is_aligned(const void *p, size_t a) { return ((uintptr_t)p % a) == 0; }

// a pair of timing events that cannot leak on an early return
struct EventPair {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t create()
    {
        hipError_t e = hipEventCreate(&e0);
        return e != hipSuccess ? e : hipEventCreate(&e1);
    }
    ~EventPair()
    {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
};


// ---- what a dispatch call is about: the colour frames, the code planes, how to launch --------------------------------------
enum class Elem { F32, F16 };   // element type of colour frames: float, or binary16 behind uint16_t
static inline size_t elem_size(Elem e) { return e == Elem::F16 ? sizeof(uint16_t) : sizeof(float); }

// nframes colour frames of w x h pixels: colour plane k of frame f at plane[k] + f * frame_stride ELEMENTS of type `elem`.
// The element type is stated here and nowhere else.  V: const void (encode sources) or void (decode destinations)
template <typename V>
struct FramesT {
    V *plane[3];
    Elem elem;
    size_t frame_stride;   // elements
    unsigned nframes, w, h;
};
using SrcFrames = FramesT<const void>;
using DstFrames = FramesT<void>;

template <typename T>
using frames_of = FramesT<std::conditional_t<std::is_const_v<T>, const void, void>>;
template <typename T>
constexpr Elem elem_of()
{
    static_assert(std::is_same_v<std::remove_const_t<T>, float> || std::is_same_v<std::remove_const_t<T>, uint16_t>, "float or binary16 frames");
    return std::is_same_v<std::remove_const_t<T>, float> ? Elem::F32 : Elem::F16;
}
// packed frames (the reference's LumaFrame): plane k at base + k * w * h; a null base gives three null planes
template <typename T>
frames_of<T> packed_frames(T *base, size_t frame_stride, unsigned nframes, unsigned w, unsigned h)
{
    const size_t n = (size_t)w * h;
    return {{base, base ? base + n : nullptr, base ? base + 2 * n : nullptr}, elem_of<T>(), frame_stride, nframes, w, h};
}
// three plane pointers; a null array gives three null planes
template <typename T>
frames_of<T> planar_frames(T *const planes[3], size_t frame_stride, unsigned nframes, unsigned w, unsigned h)
{
    return {{planes ? planes[0] : nullptr, planes ? planes[1] : nullptr, planes ? planes[2] : nullptr}, elem_of<T>(), frame_stride, nframes, w, h};
}
// rows [r0, r0 + rows) of every plane (the row bands of the host entry points)
template <typename V>
FramesT<V> row_band(FramesT<V> f, unsigned r0, unsigned rows)
{
    using B = std::conditional_t<std::is_const_v<V>, const unsigned char, unsigned char>;
    for (auto &p : f.plane)
        p = static_cast<B *>(p) + (size_t)r0 * f.w * elem_size(f.elem);
    f.h = rows;
    return f;
}
static inline SrcFrames readonly(const DstFrames &f) { return {{f.plane[0], f.plane[1], f.plane[2]}, f.elem, f.frame_stride, f.nframes, f.w, f.h}; }

// the code planes of the same frames, by reference to the caller's arrays (any of them may be null: the dispatch functions
// check).  B: unsigned char (encode destinations) or const unsigned char (decode sources)
template <typename B>
struct CodePlanesT {
    B *const *planes;      // [3]
    const int *stride;     // [3], bytes
    const size_t *pfs;     // [3], bytes from one frame's plane to the next frame's
    int profile;
};
using DstPlanes = CodePlanesT<unsigned char>;
using SrcPlanes = CodePlanesT<const unsigned char>;

// Where binary16 source frames come from (read only when the frames' element type is F16):
//   Typed   the caller's frames are binary16 by type (the _f16 entry points): every search mode and width, the YCbCr half-input
//           table whenever it exists for (sc, maxLum) and no statistics are asked for -- no probe, no feedback, no host wait;
//   Upload  this library's half upload produced them from float frames (lumahip_host.hip xfer_h2d_f16):
//           LUMAHIP_ERR_UNSUPPORTED unless encode_supports_in16() (records in LDS, rows of a multiple of 4 pixels)
enum class HalfSource { Typed, Upload };

// cs_eff: the colour space the kernels run (the context's, or CS_PACK / CS_RGB for the pack-only entry points).
// stream: where the kernels -- and any table built for them on the way -- are queued: the context's stream, or the kernel
// stream of a host entry point's pipeline.
// lanes: the call is one of the _device encode / decode entry points and goes to a lane of an open unordered section instead;
// every other caller (the _host entry points with their own upload / kernel / download streams, the stream push / pop, the
// display decode) stays on `stream` whether a section is open or not, as include/lumahip.h promises
struct EncodeLaunch {
    int cs_eff;
    hipStream_t stream;
    bool lanes = false;
    HalfSource halves = HalfSource::Typed;
};
struct DisplayParams {
    unsigned char *rgba = nullptr;
    int stride = 0;
    size_t frame_stride = 0;
    float exposure = 1.0f, gamma = 2.2f;
    int do_tmo = 0, ldr_sim = 0;
};
struct DecodeLaunch {
    int cs_eff;
    hipStream_t stream;
    bool lanes = false;
    // PACKED float frames rotating over three buffers, frame f at rot[f % 3] + (f / 3) * frame_stride (the frames' planes are
    // then ignored); not with binary16 frames or a display output
    float *const *rot = nullptr;
    const DisplayParams *display = nullptr;   // + the display epilogue; not with binary16 frames
};

// ---- lumahip_launch.hip
static inline size_t lut_lds_bytes(const QuantDev &q) { return ((size_t)(q.lut_len + q.pad) * 4 + 15) & ~(size_t)15; }   // the luminance table, or the y table, in LDS
size_t lds_bytes(const lumahip_ctx *c, bool encode_side, int cs_eff, bool ycode = false, bool half = false);   // ycode: the composite-record encode kernels; half: + the half-input table
int block_threads_for(const lumahip_ctx *c, size_t lds, bool few_waves = false, bool valu_bound = false);
int grid_for(const lumahip_ctx *c, int threads, int total_tiles, int dir, int few_writers = 0, int ycbcr = 0, bool transcode = false, int own_per_cu = 0);   // few_writers: 0 no, 1 yes, 2 yes with the colour planes in separate buffers; ycbcr: 0 no, 1 yes, 2 the half-input encode kernels; transcode: the k_transcode family (dir 0); own_per_cu > 0: this family's own workgroups per CU in the place of the rules' (the tune keys keep their precedence)
// ---- lumahip_core.hip
int ensure_search_index(lumahip_ctx *c, hipStream_t s);   // every encode-side launch calls this first (lazy build / process-wide cache); s: the stream that launch goes to
bool ycbcr_composite_ready(const lumahip_ctx *c);   // encode: the composite luma -> code records exist and fit LDS
int half_table_for(lumahip_ctx *c, float sc, const float **tab);   // *tab = the device half-input table of (sc, the quantizer's Lmax), or nullptr: none
// this eligible launch: the data-dependent ("fast") kernel (true) or the plain one.  On true, *flag is the launch's feedback
// word (nullptr when the feedback ring could not be set up: the policy then always answers true) and the caller calls
// lag_policy_launched(c, p, stream) right behind the kernel launch.
// lag_policy_next may BLOCK the calling thread: it reads the word of the fast launch issued LAG eligible launches earlier after
// waiting for that launch's event (hipEventSynchronize, not a poll: what the policy decides must be a function of the data, never
// of how far the device has got).  At most LAG - 1 eligible launches of a context are therefore queued behind the one being
// waited for -- 3 x 0.4 ms of work at 20 4K frames per launch, 3 x 21 us at one frame against a 6 us launch cost: the device
// does not run dry; include/lumahip.h says so at the *_device entry points.
bool lag_policy_next(LagPolicy &p, uint32_t **flag);
int lag_policy_launched(lumahip_ctx *c, LagPolicy &p, hipStream_t s);
void lag_policy_cancel(LagPolicy &p);   // the launch lag_policy_next handed a word to did not happen: forget its pending entry
struct LagLaunchGuard {                 // cancels on every return between lag_policy_next and the kernel launch
    LagPolicy &p;
    uint32_t *flag;
    bool launched = false;
    ~LagLaunchGuard()
    {
        if (flag && !launched)
            lag_policy_cancel(p);
    }
};
void lag_policy_reset(LagPolicy &p);      // a new stream: waits for the launches in flight, clears their words, state ON_FAST
void lag_policy_destroy(LagPolicy &p);
void numa_resolve(lumahip_ctx *c);                                 // fills numa_node / numa_cpus once (cheap afterwards)
int check_geom(lumahip_ctx *c, unsigned w, unsigned h, int profile, int cs_eff);
bool make_geom(FrameGeom &g, unsigned w, unsigned h, int vw, int nw, unsigned nframes);
hipStream_t launch_stream(lumahip_ctx *c, hipStream_t s, bool lanes);   // s, or -- for the entry points that take part in unordered sections -- the next lane of an open one
void plane_dims(unsigned w, unsigned h, int profile, int p, int &rows, int &row_bytes);
// the code planes' strides against f's geometry and, with `overlap_test`, that no two colour planes of f overlap
int check_layout(lumahip_ctx *c, const SrcFrames &f, bool overlap_test, const int stride[3], const size_t pfs[3], int profile);
// bytes plane p covers over the batch: up to the end of its last row in the last frame
static inline size_t plane_extent(unsigned w, unsigned h, int profile, int p, int stride, size_t pfs, unsigned nframes)
{
    int rows, row_bytes;
    plane_dims(w, h, profile, p, rows, row_bytes);
    return (size_t)(nframes - 1) * pfs + (size_t)(rows - 1) * (size_t)stride + (size_t)row_bytes;
}
static inline size_t round16(size_t b) { return (b + 15) & ~(size_t)15; }
static inline bool ranges_overlap(uintptr_t a, size_t na, uintptr_t b, size_t nb) { return a < b + nb && b < a + na; }

// ---- what a measuring launch delivers: the one record every measuring call builds, once, from its kind, its name in messages, its
// block and its geometry, and hands to its plan, its closing launch and (the host forms) its staging.
//   Frame    12 words per frame (block ignored), zeroed in front of the launch, 16 words of LDS to meet in;
//   Map      the distortion map -- blocks of 16, 32 or 64 luma pixels, 12 words each, every one written by the launch,
//            lh::DIST_MAP_LDS_WORDS of LDS;
//   Moments  the moments map -- blocks of 8, 16, 32 or 64, 15 words each, every one written by the launch, lh::MOMENTS_MAP_LDS_WORDS;
//   Light    the content light level -- lh::LIGHT_WORDS words per frame (block ignored), zeroed in front of the launch, as many of LDS.
enum class DistWhat { Frame, Map, Moments, Light };
struct MeasureOut {
    DistWhat kind;
    const char *call;   // in messages: "distortion map", "transcode moments map", "planes distortion", ...
    unsigned block, nframes, w, h;
    MeasureOut(DistWhat kind_, const char *call_, unsigned block_, unsigned nframes_, unsigned w_, unsigned h_)
        : kind(kind_), call(call_), block(kind_ == DistWhat::Map || kind_ == DistWhat::Moments ? block_ : 0), nframes(nframes_), w(w_), h(h_)
    {
    }
    bool map() const { return kind == DistWhat::Map || kind == DistWhat::Moments; }
    bool block_ok() const { return !map() || block == 16 || block == 32 || block == 64 || (kind == DistWhat::Moments && block == 8); }
    // the first error of every call that takes a block
    int check_block(lumahip_ctx *c) const
    {
        return block_ok() ? LUMAHIP_OK
                          : fail(c, LUMAHIP_ERR_ARG, "%s: block must be %s16, 32 or 64 (got %u)", call, kind == DistWhat::Moments ? "8, " : "", block);
    }
    unsigned nbx() const { return (w + block - 1) / block; }   // (of a map with a valid block)
    unsigned nby() const { return (h + block - 1) / block; }
    size_t words_per_block() const { return kind == DistWhat::Moments ? 15 : 12; }
    size_t words_per_frame() const { return map() ? (size_t)nbx() * nby() * words_per_block() : kind == DistWhat::Light ? (size_t)LIGHT_WORDS : 12; }
    size_t words() const { return (size_t)nframes * words_per_frame(); }
    size_t bytes() const { return words() * sizeof(uint64_t); }
    const char *out_name() const { return kind == DistWhat::Moments ? "mom_dev" : kind == DistWhat::Map ? "map_dev" : "out_dev"; }
    // the words the waves of a workgroup meet in (static LDS of the kernels, counted in every LDS budget)
    size_t lds_bytes() const
    {
        return (kind == DistWhat::Moments ? (size_t)MOMENTS_MAP_LDS_WORDS : kind == DistWhat::Map ? (size_t)DIST_MAP_LDS_WORDS
                : kind == DistWhat::Light ? (size_t)LIGHT_WORDS : 16) * sizeof(uint64_t);
    }
    bool zeroed() const { return !map(); }   // in front of the launch; a map's words are all written by it
    // the two maps: the 2 NW rows of a standard tile divide the block (every workgroup size is a power of two)
    int clamp_threads(int threads) const { return map() ? std::min(threads, 32 * (int)block) : threads; }
    // out: non-null and 8-byte aligned
    int check_out(lumahip_ctx *c, const uint64_t *out) const
    {
        return (!out || !is_aligned(out, 8)) ? fail(c, LUMAHIP_ERR_ARG, "%s must be non-null and 8-byte aligned", out_name()) : LUMAHIP_OK;
    }
};

// ---- the checks the plans of the measuring calls (and of the transcode) share
// a set of code planes a launch reads and what its planes are called in messages: pre + "plane k" + post
struct PlaneSet {
    const SrcPlanes &p;
    const char *pre = "", *post = "";
    unsigned w = 0, h = 0;   // the set's own size where it is not the record's (the source set of the half-resolution calls); 0: the record's
};
// every set's three arrays (and whatever else the family wants non-null: others_given) -> "null argument"; then plane k of every set
static inline int check_plane_sets(lumahip_ctx *c, std::initializer_list<PlaneSet> sets, bool others_given)
{
    for (const PlaneSet &s : sets)
        others_given = others_given && s.p.planes && s.p.stride && s.p.pfs;
    if (!others_given)
        return fail(c, LUMAHIP_ERR_ARG, "null argument");
    for (int k = 0; k < 3; k++)
        for (const PlaneSet &s : sets)
            if (!s.p.planes[k])
                return fail(c, LUMAHIP_ERR_ARG, "null plane %d", k);
    return LUMAHIP_OK;
}
// check_geom's tests of the size and of the profile, without its demand for a quantizer
static inline int check_size(lumahip_ctx *c, unsigned w, unsigned h)
{
    return (w == 0 || h == 0 || (w & 1) || (h & 1)) ? fail(c, LUMAHIP_ERR_ARG, "Invalid frame size %ux%u (must be even, non-zero)", w, h) : LUMAHIP_OK;
}
static inline int check_profile(lumahip_ctx *c, int profile)
{
    return (profile < 0 || profile > 3) ? fail(c, LUMAHIP_ERR_ARG, "profile must be 0..3 (got %d)", profile) : LUMAHIP_OK;
}
// a plane set's strides and frame strides against (nframes, w, h)
static inline int check_planes_layout(lumahip_ctx *c, const SrcPlanes &p, unsigned nframes, unsigned w, unsigned h)
{
    const SrcFrames geom{{nullptr, nullptr, nullptr}, Elem::F32, 0, nframes, w, h};   // (check_layout reads the geometry only)
    return check_layout(c, geom, false, p.stride, p.pfs, p.profile);
}
// The words may not share a byte with anything the launch reads, judged by the byte count of what it writes: colour plane k of the
// frames (f may be null), then plane k of every set, k = 0, 1, 2
static inline int check_out_overlap(lumahip_ctx *c, const MeasureOut &m, const uint64_t *out, const SrcFrames *f, std::initializer_list<PlaneSet> sets)
{
    const size_t frame_span = f ? ((size_t)(m.nframes - 1) * f->frame_stride + (size_t)m.w * m.h) * elem_size(f->elem) : 0;
    for (int k = 0; k < 3; k++) {
        if (f && ranges_overlap((uintptr_t)out, m.bytes(), (uintptr_t)f->plane[k], frame_span))
            return fail(c, LUMAHIP_ERR_ARG, "%s overlaps colour plane %d of the frames", m.out_name(), k);
        for (const PlaneSet &s : sets)
            if (ranges_overlap((uintptr_t)out, m.bytes(), (uintptr_t)s.p.planes[k],
                               plane_extent(s.w ? s.w : m.w, s.h ? s.h : m.h, s.p.profile, k, s.p.stride[k], s.p.pfs[k], m.nframes)))
                return fail(c, LUMAHIP_ERR_ARG, "%s overlaps %splane %d%s", m.out_name(), s.pre, k, s.post);
    }
    return LUMAHIP_OK;
}
// every base, stride and frame stride of these planes takes the vector accesses of VW pixels per thread and row
template <typename B>
static inline bool planes_aligned(const CodePlanesT<B> &p, int vw)
{
    const bool sub = (p.profile == 0 || p.profile == 2);
    const int bps = p.profile > 1 ? 2 : 1;
    for (int k = 0; k < 3; k++) {
        const size_t ub = (size_t)((k && sub) ? vw / 2 : vw) * bps;
        if (!is_aligned(p.planes[k], ub) || (p.stride[k] % (int)ub) != 0 || (p.pfs[k] % ub) != 0)
            return false;
    }
    return true;
}

// code planes a kernel reads, as its DecArgs names them (the transcode's source planes, the given planes of both measuring calls)
static inline void read_planes(DecArgs &d, const SrcPlanes &p, int vw)
{
    d.bps = p.profile > 1 ? 2 : 1;
    d.aligned = planes_aligned(p, vw) ? 1 : 0;
    for (int k = 0; k < 3; k++) {
        d.src[k] = p.planes[k];
        d.stride[k] = p.stride[k];
        d.src_frame_stride[k] = p.pfs[k];
    }
}
// The colour planes of frames with elements of esz bytes: loads of two pixels need 2-element alignment, else the call is refused;
// *al4: rows, planes and frame stride also take the loads of four
static inline int check_frame_alignment(lumahip_ctx *c, const SrcFrames &f, size_t esz, bool *al4)
{
    auto al = [&](size_t n) { return is_aligned(f.plane[0], n * esz) && is_aligned(f.plane[1], n * esz) && is_aligned(f.plane[2], n * esz) && (f.frame_stride % n) == 0; };
    *al4 = (f.w % 4) == 0 && al(4);
    return al(2) ? LUMAHIP_OK : fail(c, LUMAHIP_ERR_ARG, "colour planes must be %d-byte aligned and the frame stride even", (int)(2 * esz));
}
// The launch of a fused kernel (+ dynamic LDS beyond 64 KiB); the caller reads hipGetLastError once all that belongs to it is queued
template <typename A>
int launch_fused(lumahip_ctx *c, void (*kern)(const A), int grid, int threads, size_t lds, hipStream_t s, const A &a)
{
    if (lds > 64 * 1024)
        HIPCHK(c, hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), lds, s, a);
    return LUMAHIP_OK;
}
// ... of a measuring kernel, the one way every measuring dispatch closes: the words at out (what the kernel's arguments name out or
// map) are zeroed in front of it where the record says so, and nothing follows it
template <typename A>
int launch_measure(lumahip_ctx *c, const MeasureOut &m, uint64_t *out, void (*kern)(const A), int grid, int threads, size_t lds, hipStream_t s,
                   const A &a)
{
    if (m.zeroed())
        HIPCHK(c, hipMemsetAsync(out, 0, m.bytes(), s));
    if (int rc = launch_fused(c, kern, grid, threads, lds, s, a))
        return rc;
    HIPCHK(c, hipGetLastError());
    return LUMAHIP_OK;
}
// What the two maps add to a plan behind grid_for (whose rule runs over the standard tiles): the map's geometry -- threads = the
// workgroup, clamped by MeasureOut::clamp_threads in front of make_geom -- and a grid of at most its tiles: a workgroup takes whole ones
static inline lh::MapGeom make_map_geom(const lh::FrameGeom &g, unsigned w, unsigned h, unsigned block, int threads)
{
    lh::MapGeom m{};
    m.B = (int)block;
    m.S = (int)block / (2 * (threads / 64));
    m.nbx = (int)((w + block - 1) / block);
    m.nby = (int)((h + block - 1) / block);
    m.mapTilesPerFrame = m.nby * g.tilesX;
    m.totalMapTiles = m.mapTilesPerFrame * g.nframes;   // (<= the standard tiles, which make_geom has bounded)
    return m;
}
static inline void map_shape(const MeasureOut &m, const lh::FrameGeom &g, int threads, lh::MapGeom &mg, int &grid)
{
    if (!m.map())
        return;
    mg = make_map_geom(g, m.w, m.h, m.block, threads);
    grid = std::min(grid, mg.totalMapTiles);
}

// How a _device dispatch is launched (the transcode and every measuring call): stream as EncodeLaunch::stream, lanes as
// EncodeLaunch::lanes
struct StreamLaunch {
    hipStream_t stream;
    bool lanes = false;
};
// What their _device entry points do in front of the dispatch: the context; args_given: the packed forms' base pointer (the planar
// forms' three pointers and the plane sets are the plans' to check)
template <typename F>
static inline int device_entry(lumahip_ctx *c, bool args_given, F dispatch)
{
    if (!c)
        return LUMAHIP_ERR_ARG;
    if (!args_given)
        return fail(c, LUMAHIP_ERR_ARG, "null argument");
    return dispatch(StreamLaunch{c->stream, true});
}

// ---- lumahip_encode.hip / lumahip_decode.hip
int encode_frames_device_impl(lumahip_ctx *c, const SrcFrames &f, float sc, const DstPlanes &p, float *stats, const EncodeLaunch &o);
bool encode_supports_in16(lumahip_ctx *c, unsigned w);
int stats_begin(lumahip_ctx *c, unsigned nframes, bool lanes, hipStream_t *s, float **part);   // the statistics scratch of a launch (lumahip_encode.hip)
void stats_fold(lumahip_ctx *c, unsigned nframes, float *stats, hipStream_t s);
int decode_impl(lumahip_ctx *c, const SrcPlanes &p, float sc, const DstFrames &f, const DecodeLaunch &o);
int rb_table_for(lumahip_ctx *c, float sc, hipStream_t s, const float **tab);   // built on s the first time a preScaling is seen
int array_launch(lumahip_ctx *c, const float *d_in, float *d_out, size_t n, unsigned ch, bool quant);
// ---- lumahip_encode_f16.hip / lumahip_decode_f16.hip: pick_enc<true> / pick_dec<true> of lumahip_pick.hpp (own translation
// units: the binary16-frame kernels compile side by side with the float ones).  nullptr: none for these arguments
typedef void (*enc_kernel_t)(const lh::EncArgs);
typedef void (*dec_kernel_t)(const lh::DecArgs);
enc_kernel_t pick_enc_f16(int cs, bool sub, int vw, int mode);
dec_kernel_t pick_dec_f16(int cs, bool sub, int vw, bool gl, bool yt, bool rb);

// ---- lumahip_transcode.hip
// source planes under the context's source quantizer and src_sc -> destination planes under its quantizer and dst_sc
int transcode_impl(lumahip_ctx *c, const SrcPlanes &src, float src_sc, unsigned nframes, unsigned w, unsigned h, const DstPlanes &dst, float dst_sc,
                   float *stats, const StreamLaunch &o);
typedef void (*trans_kernel_t)(const lh::TransArgs);
// What transcode_plan decides for a launch over (source planes, target-side planes): the kernel's key (colour spaces,
// subsamplings, vector width, the target's search mode as pick_planes takes it), the launch shape and the kernel arguments of both
// sides except the target-side plane pointers, which the two callers fill in (written: EncArgs::dst; read: a DecArgs of their own)
struct TranscodePlan {
    int csd, cse, kmode, vw, threads, grid;
    bool subd, sube, any_y;
    size_t lds;      // dynamic LDS of the launch (the measuring kernels' words are static and counted in the budget)
    lh::DecArgs d;   // q, g, src, stride, src_frame_stride, sc, bps, aligned of the source planes
    lh::EncArgs e;   // q (the composite records for kmode 5), g (d's; scale 2 / 4: of the half-size / quarter-size target), sc, bps, aligned of the target side
    lh::MapGeom m;   // the two maps only
};
// m == nullptr, the storing transcode: tgt are the planes lumahip_transcode_frames_device writes (no source plane may overlap one),
// out is ignored; scale 2 or 4: the half- / quarter-resolution transcode, tgt of (w / scale) x (h / scale), the workgroup clamped to
// lh::transhalf_threads_bound / lh::transquarter_threads_bound.  Else a measuring call and what it delivers (MeasureOut; its nframes, w, h are the target side's: the arguments', or
// with scale 2 -- the half-resolution transcode distortion and its map -- w / 2 and h / 2, and the workgroup is then clamped to
// lh::transhalfdist_threads_bound / lh::transhalfmap_threads_bound and the vector width held to lh::transhalfdist_vw4): tgt are the given
// planes (read only: any overlap with the source is fine), out its words (non-null, 8-byte aligned, sharing no byte with either plane
// set), the workgroup is clamped to the measuring kernels' launch bound -- the moments map's: to lh::transmoments_threads_bound in its
// place -- and, the two maps, by the record's rule; their grid to the number of map tiles.  Every error is raised here, the block
// size first, before anything of the launch is queued.
int transcode_plan(lumahip_ctx *c, const SrcPlanes &src, float src_sc, unsigned nframes, unsigned w, unsigned h, const SrcPlanes &tgt, float dst_sc,
                   const MeasureOut *m, const uint64_t *out, hipStream_t stream, TranscodePlan &p, unsigned scale = 1);
// ---- lumahip_transcode_half.hip: pick_planes<TransHalfFamily, .> (every k_transcode_half), the dispatch and its entry point
// source planes of w x h -> destination planes of (w/2) x (h/2): the 2x2 box in linear light between the decode and the encode
int transcode_half_impl(lumahip_ctx *c, const SrcPlanes &src, float src_sc, unsigned nframes, unsigned w, unsigned h, const DstPlanes &dst, float dst_sc,
                        float *stats, const StreamLaunch &o);
// ---- lumahip_transcode_quarter.hip: pick_planes<TransQuarterFamily, .> (every k_transcode_quarter), the dispatch and its entry point
// source planes of w x h -> destination planes of (w/4) x (h/4): the 2x2 box in linear light twice, on floats, between the decode and the encode
int transcode_quarter_impl(lumahip_ctx *c, const SrcPlanes &src, float src_sc, unsigned nframes, unsigned w, unsigned h, const DstPlanes &dst, float dst_sc,
                           float *stats, const StreamLaunch &o);
// the decoded and colour-transformed channel 0 of ONE frame (w*h floats at out_dev), with the complete per-pixel functions
int transcode_channel0(lumahip_ctx *c, const SrcPlanes &src, float src_sc, unsigned w, unsigned h, float dst_sc, float *out_dev, hipStream_t s);

// ---- lumahip_distortion.hip: the frame-fed measuring calls
// What distortion_plan decides for a launch that scores given planes against the frames' encode: the kernel's key as pick_dist
// takes it, the launch shape and the kernel arguments of both sides
struct DistortionPlan {
    int cs, kmode, vw, threads, grid;
    bool sub, in16;
    size_t lds;      // dynamic LDS of the launch (the words the waves meet in are static and counted in the budget)
    lh::EncArgs e;   // DistArgs::e
    lh::DecArgs g;   // DistArgs::g
    lh::MapGeom m;   // the two maps only
};
// m: what the launch delivers (its nframes, w, h are f's); out: its words (non-null, 8-byte aligned, sharing no byte with the frames
// or the given planes); the workgroup of the two maps is clamped by the record's rule (a map tile is a whole number of standard
// tiles), the moments map's also to its kernels' launch bound (lh::moments_threads_bound).  Every error is raised here, the block
// size first, before anything of the launch is queued.
int distortion_plan(lumahip_ctx *c, const SrcFrames &f, float sc, const SrcPlanes &given, const MeasureOut &m, const uint64_t *out,
                    hipStream_t stream, DistortionPlan &p);

// The one dispatch of the frame-fed measuring calls: the frames of f under the context's quantizer and sc against the given planes,
// m.words() words at out
int measure_frames_impl(lumahip_ctx *c, const SrcFrames &f, float sc, const SrcPlanes &given, const MeasureOut &m, uint64_t *out,
                        const StreamLaunch &o);
// pick_dist<Family, IN16> of lumahip_pick.hpp as the six kernel units export it (each compiles the kernels it names, side by side with
// the others): lumahip_distortion.hip / _f16.hip, lumahip_distortion_map.hip / _f16.hip, lumahip_moments_map.hip / _f16.hip
typedef void (*dist_kernel_t)(const lh::DistArgs);
typedef void (*map_kernel_t)(const lh::MapArgs);
dist_kernel_t pick_dist_f32(int cs, bool sub, int vw, int mode), pick_dist_f16(int cs, bool sub, int vw, int mode);
map_kernel_t pick_dist_map_f32(int cs, bool sub, int vw, int mode), pick_dist_map_f16(int cs, bool sub, int vw, int mode);
map_kernel_t pick_moments_map_f32(int cs, bool sub, int vw, int mode), pick_moments_map_f16(int cs, bool sub, int vw, int mode);

// ---- lumahip_transcode.hip: the plane-fed measuring calls
// The size of a measuring call's source set where it is not the record's: the half-resolution calls (scale 2), whose record and
// given set are of (w / 2) x (h / 2)
struct SourceSize {
    unsigned w, h, scale;
};
// The one dispatch of the five: the source planes' transcode (transcode_impl's planes, never written) against the given planes,
// m.words() words at out; m carries nframes, w, h.  full: the source's size of the two half-resolution calls, whose e is
// transcode_half_impl's sample
int measure_planes_impl(lumahip_ctx *c, const SrcPlanes &src, float src_sc, const SrcPlanes &given, float dst_sc, const MeasureOut &m, uint64_t *out,
                        const StreamLaunch &o, const SourceSize *full = nullptr);
// pick_planes<TransDistFamily | TransDistMapFamily | TransMomentsMapFamily, vw> of lumahip_pick.hpp as lumahip_transcode_distortion.hip /
// lumahip_transcode_distortion_map.hip / lumahip_transcode_moments_map.hip export it (each compiles the 48 kernels it names)
typedef void (*transdist_kernel_t)(const lh::TransDistArgs);
typedef void (*transdist_map_kernel_t)(const lh::TransDistMapArgs);
transdist_kernel_t pick_transdist(int vw, int csd, bool subd, int cse, bool sube, int mode);
transdist_map_kernel_t pick_transdist_map(int vw, int csd, bool subd, int cse, bool sube, int mode);
transdist_map_kernel_t pick_transdist_moments_map(int vw, int csd, bool subd, int cse, bool sube, int mode);
// pick_planes<TransHalfDistFamily | TransHalfDistMapFamily, vw> as lumahip_transcode_half_distortion.hip /
// lumahip_transcode_half_distortion_map.hip export it (each compiles the kernels it names)
transdist_kernel_t pick_transhalf_dist(int vw, int csd, bool subd, int cse, bool sube, int mode);
transdist_map_kernel_t pick_transhalf_dist_map(int vw, int csd, bool subd, int cse, bool sube, int mode);

// ---- lumahip_planes_measure.hip: two plane sets as they are (include/lumahip_compare.h)
// e = the samples of set a, g = those of set b (one profile, which both sets carry), no quantizer read; m.words() words at out, m
// carries nframes, w, h.  Every error is raised before anything is queued, the block size first.
int planes_measure_impl(lumahip_ctx *c, const SrcPlanes &a, const SrcPlanes &b, const MeasureOut &m, uint64_t *out, const StreamLaunch &o);

// ---- lumahip_light_level.hip: the content light level of frames or of code planes (include/lumahip_compare.h)
// Exactly one of f (frames as they are; no quantizer read, sc ignored) and pl (code planes under the context's quantizer and sc) is
// non-null; m (DistWhat::Light) carries nframes, w, h; m.words() words at out.  Every error is raised before anything is queued.
int light_level_impl(lumahip_ctx *c, const SrcFrames *f, const SrcPlanes *pl, float sc, float scale, const MeasureOut &m, uint64_t *out,
                     const StreamLaunch &o);
// its test of the caller's scale (the host forms ask it too: nothing of a refused call is uploaded)
static inline int check_light_scale(lumahip_ctx *c, float scale)
{
    return (!(scale > 0.0f) || !std::isfinite(scale)) ? fail(c, LUMAHIP_ERR_ARG, "light level: scale must be finite and > 0 (got %g)", (double)scale)
                                                      : LUMAHIP_OK;
}

// ---- lumahip_misc.hip
int seq_mean(lumahip_ctx *c, const float *chan0_dev, unsigned w, unsigned h, float *mean_host);
int mean_luminance_reference_impl(lumahip_ctx *c, const void *rgb_dev, Elem elem, unsigned w, unsigned h, float sc, int cs_eff,
                                  float *mean_host);   // one packed frame of `elem` at rgb_dev

// ---- lumahip_host.hip
int xfer_h2d(lumahip_ctx *c, void *dst, const void *src, size_t bytes, hipStream_t s);
int xfer_d2h(lumahip_ctx *c, void *dst, const void *src, size_t bytes, hipStream_t s);
int read_small(lumahip_ctx *c, float *dst, const float *src_dev, int n, hipStream_t s);
int ensure(lumahip_ctx *c, void **p, size_t *cap, size_t need);

}  // namespace lhost
