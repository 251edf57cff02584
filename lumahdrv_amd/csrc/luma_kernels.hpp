// luma_kernels.hpp -- fused encode / decode kernels of the Luma HDRv quantize / dequantize path, gfx950.
//
// ENC = LumaQuantizer::transformColorSpace(frame,true,sc) (src/luma_quantizer.cpp:267-373) fused with
//       LumaEncoder::setChannels / setVpxChannel (src/luma_encoder.cpp:196-201,260-317);
// DEC = LumaDecoder::getVpxChannels (src/luma_decoder.cpp:205-240) fused with
//       LumaQuantizer::transformColorSpace(frame,false,sc) (src/luma_quantizer.cpp:374-479).
//
// Work decomposition (both directions): a *unit* is VW pixels x 2 rows (VW/2 chroma quads in 4:2:0); a
// thread owns one unit per tile; a wave owns 64 consecutive units of one row pair (64*VW*4 B = 1 KiB
// contiguous per load instruction per row and channel); a workgroup of NW waves owns a tile of
// 64*VW pixels x 2*NW rows; workgroups are persistent and stride over tiles (tile index is
// wave-uniform, so all index arithmetic on it is scalar).  The luminance search records (encode) /
// the transfer-function table (decode) are staged once per workgroup in LDS.  No inter-workgroup communication except the optional
// per-frame statistics (float atomics).
#pragma once

#include <type_traits>

#include "f16_narrow.hpp"
#include "luma_device.hpp"


namespace lh {

// Minimum waves per SIMD the encode kernels are register-allocated for.  The light variants (Lu'v' / pack-only,
// 4:2:0 or VW=2) fit 80 VGPRs without spilling and run 6 waves per SIMD; the heavy ones (fp64 powf, three LUT
// searches per pixel, 4:4:4 with VW=4) would spill at that bound and keep the 4-wave / 128-VGPR budget.
template <int CS, bool SUB, int VW>
struct EncWaves {
    static constexpr int value = ((CS == CS_LUV || CS == CS_PACK) && (SUB || VW == 2)) ? 6 : 4;
};

struct FrameGeom {
    int w, h;            // luma size (even)
    int unitsX, unitsY;  // w/VW, h/2
    int tilesX, tilesY;  // ceil(unitsX/64), ceil(unitsY/NW)
    int tilesPerFrame;
    int totalTiles;      // tilesPerFrame * nframes
    int nframes;
    int interleave;      // 0: tiles in frame-major order; 1: tile t belongs to frame t % nframes (DecArgs::rot says why)
};

struct EncArgs {
    QuantDev q;
    FrameGeom g;
    const float *src[3];  // colour plane c of frame f at src[c] + f*frame_stride (the reference's LumaFrame,
                          // include/luma/luma_frame.h:84-87 there, is src[c] = base + c*w*h, frame_stride = 3*w*h)
    size_t frame_stride;  // floats
    unsigned char *dst[3];
    int stride[3];        // bytes
    size_t dst_frame_stride[3];
    float sc;
    int bps;              // bytes per sample: 1 or 2
    int aligned;          // 1: vector stores allowed
    float *stats;         // nullable: per frame STATS_SLOTS partial {sum,min,max} triples (k_fold_stats folds them)
    const float *half;    // LM == 6 only: the half-input table of this (sc, Lmax), HALF_TABLE_LEN floats padded to 16 B (luma_device.hpp half_lookup)
    // LM == 6 only, nullable: THIS launch's word in host-visible memory, which a workgroup sets to 1 when every unit of every
    // one of its waves held inputs that are not halves -- the stream is not binary16 data and the host stops picking this
    // kernel for a while (LagPolicy, lumahip_internal.hpp: the host reads the word after the launch's completion event).  Feedback only:
    // nothing a launch computes depends on it.
    uint32_t *half_flag;
};

struct DecArgs {
    QuantDev q;
    FrameGeom g;
    const unsigned char *src[3];
    int stride[3];
    size_t src_frame_stride[3];
    float *dst[3];        // colour plane c of frame f at dst[c] + f*frame_stride; dst[0] null when only the display output is wanted
    size_t frame_stride;
    // rot_on: PACKED frames (LumaFrame layout, channel c at base + c*w*h) spread over three buffers, frame f at
    // rot[f % 3] + (f / 3) * frame_stride -- with the three buffers in three HBM region groups and the tiles of a launch interleaved
    // over its frames (FrameGeom::interleave), the workgroups running at any moment write all three groups, which one launch
    // that writes a batch of packed frames into ONE buffer cannot (lumahip_decode_frames_device_rotating)
    float *rot[3];
    int rot_on;
    float sc;
    int bps;
    int aligned;
    // optional display epilogue (lumaplay's fragment shader, src/lumaplay_dequantizer.frag:145-156):
    // RGBA8, 4 bytes per pixel, rows disp_stride bytes apart
    unsigned char *disp;
    int disp_stride;
    size_t disp_frame_stride;
    float exposure, inv_gamma;
    int do_tmo, ldr_sim;
    // YCbCr decode with the per-stream red / blue tables (k_decode<..., RB>): rb[cb * lut_len + ycode] = blue,
    // rb[rb_plane + cr * lut_len + ycode] = red, final values (after / sc) of this call's preScaling; global memory (L2 / MALL)
    const float *rb;
    size_t rb_plane;
    // a wave takes the gathers for a unit only when most of its lanes' codes are close to each other and to their neighbour
    // lane's (rb_wave_local): luminance codes within rb_near_y, colour codes within rb_near_c; negative rb_near_y: always
    int rb_near_y, rb_near_c;
    // nullable: THIS launch's word in host-visible memory, set to 1 by every workgroup in which some wave took the tables for some
    // unit -- a launch that leaves it 0 found none of its pixels local, and the host sends the next launches to the kernels
    // without the test (lumahip_internal.hpp LagPolicy).  Feedback only.
    uint32_t *rb_flag;
};

// LDS layout: [powf tables (YCbCr only; FIRST, so that their addresses are immediates in the powf chains)]
// [lut: lut_len+pad floats, rounded to 16 B | records: nbuckets u32, rounded to 16 B]
// [YCbCr decode with per-stream tables: y table (as long as the lut), then the Cb and Cr chroma-term tables, maxC+1 floats each]
// [u'v' table: maxC+1 floats (Lu'v' decode only), see luv_chroma_uv | half-input table (YCbCr encode, LM == 6)].
// Which parts a kernel stages is a compile-time set (encode: records; decode: the table; transcode: both sides, the two-quantizer
// stage_tables below).
// STAGE_POWFN: the 768-byte powf tables instead of the wide ones (the half-input kernels: their LDS belongs to the half table).
enum : int { STAGE_LUT = 1, STAGE_REC = 4, STAGE_POWF = 8, STAGE_UV = 16, STAGE_YT = 32, STAGE_POWFN = 64, STAGE_HALF = 128, STAGE_CT = 256 };

// fill the LDS copy of the powf tables (pow_glibc.hpp); the caller synchronises
LH_DEV void stage_powf_tables(PowfTables *t)
{
    const double lt[16][2] = LH_POWF_LOG2_TAB;
    const uint64_t et[32] = LH_POWF_EXP2_TAB;
    const int tid = threadIdx.x;
    if (tid < 16) {
        t->log2_tab[tid][0] = lt[tid][0];
        t->log2_tab[tid][1] = lt[tid][1];
    }
    if (tid < 32)
        t->exp2_tab[tid] = et[tid];
}
LH_DEV void stage_powf_tables(PowfTablesWide *t)
{
    const double lt[16][2] = LH_POWF_LOG2_TAB;
    stage_powf_tables(static_cast<PowfTables *>(t));
    for (int e = threadIdx.x; e < 2048; e += blockDim.x)
        pw_wide_entry(e, lt, t->wide[e][0], t->wide[e][1]);
    for (int e = threadIdx.x; e < FOLD_A_LEN; e += blockDim.x)
        pw_fold_entry<0>(e, lt, t->foldA[e][0], t->foldA[e][1]);
    if (threadIdx.x < 16)
        pw_fold_entry<1>(threadIdx.x, lt, t->foldC[threadIdx.x][0], t->foldC[threadIdx.x][1]);
}

LH_DEV int lds_lut_bytes(const QuantDev &q) { return ((q.lut_len + q.pad) * 4 + 15) & ~15; }
LH_DEV int lds_rec_bytes(const QuantDev &q) { return (q.nbuckets * (q.mode == 7 ? 8 : 4) + 15) & ~15; }   // (7: {T, start} pairs)

// offset of the search table / records behind the powf tables
template <int WHAT>
constexpr int lds_table_offset()
{
    return (WHAT & STAGE_POWF) ? (int)sizeof(PowfTablesWide) : (WHAT & STAGE_POWFN) ? (int)sizeof(PowfTables) : 0;
}

constexpr int lds_half_bytes() { return (HALF_TABLE_LEN * 4 + 15) & ~15; }

template <int WHAT>
LH_DEV void stage_tables(unsigned char *smem, const QuantDev &q, const float *half = nullptr)
{
    static_assert(sizeof(PowfTablesWide) % 16 == 0 && sizeof(PowfTables) % 16 == 0, "the tables behind the powf tables must stay 16-byte aligned");
    static_assert(!((WHAT & STAGE_LUT) && (WHAT & STAGE_REC)), "one search table per kernel");
    static_assert(!((WHAT & STAGE_POWF) && (WHAT & STAGE_POWFN)), "one set of powf tables per kernel");
    const int tid = threadIdx.x, nt = blockDim.x;
    constexpr int off = lds_table_offset<WHAT>();
    if constexpr (WHAT & STAGE_POWF)
        stage_powf_tables(reinterpret_cast<PowfTablesWide *>(smem));
    if constexpr (WHAT & STAGE_POWFN)
        stage_powf_tables(reinterpret_cast<PowfTables *>(smem));
    if constexpr (WHAT & STAGE_HALF) {
        static_assert((WHAT & STAGE_REC) && !(WHAT & (STAGE_UV | STAGE_YT)), "the half-input table sits behind the records");
        const float4 *g = reinterpret_cast<const float4 *>(half);
        float4 *s4 = reinterpret_cast<float4 *>(smem + off + lds_rec_bytes(q));
        for (int i = tid; i < lds_half_bytes() / 16; i += nt)
            s4[i] = g[i];
    }
    if constexpr (WHAT & STAGE_LUT) {
        // table length + pad is a multiple of 4 floats on the host side (buffer is padded to 16 B)
        const int n4 = lds_lut_bytes(q) / 16;
        const float4 *g = reinterpret_cast<const float4 *>(q.lut);
        float4 *s = reinterpret_cast<float4 *>(smem + off);
        for (int i = tid; i < n4; i += nt)
            s[i] = g[i];
    }
    if constexpr (WHAT & STAGE_REC) {
        const int b4 = lds_rec_bytes(q) / 16;  // the device buffer is padded to 16 B
        const uint4 *gb = reinterpret_cast<const uint4 *>(q.rec);
        uint4 *sb = reinterpret_cast<uint4 *>(smem + off);
        for (int i = tid; i < b4; i += nt)
            sb[i] = gb[i];
    }
    if constexpr (WHAT & STAGE_YT) {
        static_assert((WHAT & STAGE_LUT) && !(WHAT & STAGE_UV), "the y table of the YCbCr decode kernels sits behind the luminance table");
        const int n4 = lds_lut_bytes(q) / 16;  // same length and padding as the luminance table
        const float4 *g = reinterpret_cast<const float4 *>(q.ytab);
        float4 *s = reinterpret_cast<float4 *>(smem + off + lds_lut_bytes(q));
        for (int i = tid; i < n4; i += nt)
            s[i] = g[i];
    }
    if constexpr (WHAT & STAGE_CT) {
        // YCbCr decode: the chroma terms of every colour code (luma_device.hpp ycbcr_chroma_term), Cb table then Cr table,
        // behind the luminance table and the y table
        static_assert((WHAT & STAGE_YT), "the chroma-term tables sit behind the y table");
        float *ct = reinterpret_cast<float *>(smem + off + 2 * lds_lut_bytes(q));
        const int n = (int)q.maxC + 1;
        for (int i = tid; i < n; i += nt) {
            ct[i] = ycbcr_chroma_term(i, q.maxC, 1.8814f);
            ct[n + i] = ycbcr_chroma_term(i, q.maxC, 1.4746f);
        }
    }
    if constexpr (WHAT & STAGE_UV) {
        static_assert(WHAT & STAGE_LUT, "the u'v' table sits behind the luminance table");
        float *uv = reinterpret_cast<float *>(smem + off + lds_lut_bytes(q));
        const int n = (int)q.maxC + 1;
        for (int i = tid; i < n; i += nt)
            uv[i] = uv_table_entry(i, q.maxC);
    }
    __syncthreads();
}

// Two quantizers in one workgroup (k_transcode): ONE copy of the powf tables when either side asks for them (first, as above),
// behind it the tables of `qa` (WHAT_A), then those of `qb` (WHAT_B) from the next 16-byte boundary on -- each side staged by
// the function above at its own base, so the layout inside a side is the one its device functions know.
// lds_quant_bytes: what a side occupies behind the powf tables
template <int WHAT>
LH_DEV int lds_quant_bytes(const QuantDev &q)
{
    static_assert(!(WHAT & STAGE_HALF), "the half-input table is not part of a two-quantizer layout");
    const int col = (((int)q.maxC + 1) * 4 + 15) & ~15;
    return ((WHAT & STAGE_LUT) ? lds_lut_bytes(q) : 0) + ((WHAT & STAGE_REC) ? lds_rec_bytes(q) : 0) + ((WHAT & STAGE_YT) ? lds_lut_bytes(q) : 0) +
           ((WHAT & STAGE_CT) ? 2 * col : 0) + ((WHAT & STAGE_UV) ? col : 0);
}
template <int WHAT_A, int WHAT_B>
LH_DEV void stage_tables(unsigned char *smem, const QuantDev &qa, const QuantDev &qb)
{
    static_assert(!((WHAT_A | WHAT_B) & (STAGE_POWFN | STAGE_HALF)), "the wide powf tables or none; no half-input table");
    constexpr int POWF = (WHAT_A | WHAT_B) & STAGE_POWF;
    stage_tables<(WHAT_A & ~STAGE_POWF) | POWF>(smem, qa);
    stage_tables<WHAT_B & ~STAGE_POWF>(smem + lds_table_offset<POWF>() + lds_quant_bytes<WHAT_A>(qa), qb);
}

// ---- sample stores / loads ------------------------------------------------------------------------
// Every frame byte is touched exactly once, so all global accesses of the pixel stream are non-temporal
// (`nt`): measured +4-5 % on the encode access pattern (profiles/r01_membench.txt).
typedef float lh_v4f __attribute__((ext_vector_type(4)));
typedef float lh_v2f __attribute__((ext_vector_type(2)));
typedef unsigned lh_v2u __attribute__((ext_vector_type(2)));

LH_DEV void nt_store_u32x2(void *p, uint32_t a, uint32_t b)
{
    lh_v2u t = {a, b};
    __builtin_nontemporal_store(t, reinterpret_cast<lh_v2u *>(p));
}
LH_DEV void nt_store_u32(void *p, uint32_t a) { __builtin_nontemporal_store(a, reinterpret_cast<uint32_t *>(p)); }
LH_DEV void nt_store_u16(void *p, uint16_t a) { __builtin_nontemporal_store(a, reinterpret_cast<uint16_t *>(p)); }
LH_DEV void nt_store_u8(void *p, unsigned char a) { __builtin_nontemporal_store(a, reinterpret_cast<unsigned char *>(p)); }

// N consecutive samples (codes) at p; bps 1 or 2; little-endian 16-bit exactly as
// src/luma_encoder.cpp:301-307 produces (bl = res/256 at +1, bh = res - bl*256 at +0); the 8-bit path
// keeps the low byte (the reference's float->unsigned char conversion, quirk 2).
template <int N>
LH_DEV void store_samples(unsigned char *p, const int (&c)[N], int bps, int aligned)
{
    if (bps == 2) {
        if (aligned) {
            if constexpr (N == 4) {
                nt_store_u32x2(p, (uint32_t)(c[0] & 0xffff) | ((uint32_t)c[1] << 16),
                               (uint32_t)(c[2] & 0xffff) | ((uint32_t)c[3] << 16));
            } else if constexpr (N == 2) {
                nt_store_u32(p, (uint32_t)(c[0] & 0xffff) | ((uint32_t)c[1] << 16));
            } else {
                nt_store_u16(p, (uint16_t)c[0]);
            }
        } else {
#pragma unroll
            for (int i = 0; i < N; i++) {
                p[2 * i] = (unsigned char)(c[i] & 0xff);
                p[2 * i + 1] = (unsigned char)((c[i] >> 8) & 0xff);
            }
        }
    } else {
        if (aligned) {
            if constexpr (N == 4) {
                nt_store_u32(p, (uint32_t)(c[0] & 0xff) | ((uint32_t)(c[1] & 0xff) << 8) |
                                    ((uint32_t)(c[2] & 0xff) << 16) | ((uint32_t)(c[3] & 0xff) << 24));
            } else if constexpr (N == 2) {
                nt_store_u16(p, (uint16_t)((c[0] & 0xff) | ((c[1] & 0xff) << 8)));
            } else {
                nt_store_u8(p, (unsigned char)(c[0] & 0xff));
            }
        } else {
#pragma unroll
            for (int i = 0; i < N; i++)
                p[i] = (unsigned char)(c[i] & 0xff);
        }
    }
}

// src/luma_decoder.cpp:222-225: buf[2x+1]*256.0f + buf[2x] (exact in fp32) or buf[x]
template <int N>
LH_DEV void load_samples(const unsigned char *p, int (&c)[N], int bps, int aligned)
{
    if (bps == 2) {
        if (aligned) {
            if constexpr (N == 4) {
                const lh_v2u v = __builtin_nontemporal_load(reinterpret_cast<const lh_v2u *>(p));
                c[0] = v.x & 0xffff; c[1] = v.x >> 16; c[2] = v.y & 0xffff; c[3] = v.y >> 16;
            } else if constexpr (N == 2) {
                const uint32_t v = __builtin_nontemporal_load(reinterpret_cast<const uint32_t *>(p));
                c[0] = v & 0xffff; c[1] = v >> 16;
            } else {
                c[0] = __builtin_nontemporal_load(reinterpret_cast<const uint16_t *>(p));
            }
        } else {
#pragma unroll
            for (int i = 0; i < N; i++)
                c[i] = (int)p[2 * i] | ((int)p[2 * i + 1] << 8);
        }
    } else {
        if (aligned) {
            if constexpr (N == 4) {
                const uint32_t v = __builtin_nontemporal_load(reinterpret_cast<const uint32_t *>(p));
                c[0] = v & 0xff; c[1] = (v >> 8) & 0xff; c[2] = (v >> 16) & 0xff; c[3] = v >> 24;
            } else if constexpr (N == 2) {
                const uint32_t v = __builtin_nontemporal_load(reinterpret_cast<const uint16_t *>(p));
                c[0] = v & 0xff; c[1] = v >> 8;
            } else {
                c[0] = p[0];
            }
        } else {
#pragma unroll
            for (int i = 0; i < N; i++)
                c[i] = p[i];
        }
    }
}

template <int VW>
LH_DEV void load_px(const float *p, float (&v)[VW])
{
    if constexpr (VW == 4) {
        const lh_v4f t = __builtin_nontemporal_load(reinterpret_cast<const lh_v4f *>(p));
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        const lh_v2f t = __builtin_nontemporal_load(reinterpret_cast<const lh_v2f *>(p));
        v[0] = t.x; v[1] = t.y;
    }
}

// the same VW pixels from a frame uploaded as binary16 (the host entry points' half upload, lumahip_host.hip): exact widening
template <int VW>
LH_DEV void load_px_h(const _Float16 *p, float (&v)[VW])
{
    typedef _Float16 lh_v4h __attribute__((ext_vector_type(4)));
    typedef _Float16 lh_v2h __attribute__((ext_vector_type(2)));
    if constexpr (VW == 4) {
        const lh_v4h t = __builtin_nontemporal_load(reinterpret_cast<const lh_v4h *>(p));
        v[0] = (float)t.x; v[1] = (float)t.y; v[2] = (float)t.z; v[3] = (float)t.w;
    } else {
        const lh_v2h t = __builtin_nontemporal_load(reinterpret_cast<const lh_v2h *>(p));
        v[0] = (float)t.x; v[1] = (float)t.y;
    }
}

// the same VW pixels narrowed to binary16 (f16_narrow: the bits of ExrInterface::floatToHalf), 8 / 4 bytes non-temporal
template <int VW>
LH_DEV void store_px_h(uint16_t *p, const float (&v)[VW])
{
    if constexpr (VW == 4) {
        typedef uint32_t lh_v2u __attribute__((ext_vector_type(2)));
        const lh_v2u t = {(uint32_t)lh::f16_narrow(v[0]) | ((uint32_t)lh::f16_narrow(v[1]) << 16),
                          (uint32_t)lh::f16_narrow(v[2]) | ((uint32_t)lh::f16_narrow(v[3]) << 16)};
        __builtin_nontemporal_store(t, reinterpret_cast<lh_v2u *>(p));
    } else {
        const uint32_t t = (uint32_t)lh::f16_narrow(v[0]) | ((uint32_t)lh::f16_narrow(v[1]) << 16);
        __builtin_nontemporal_store(t, reinterpret_cast<uint32_t *>(p));
    }
}

template <int VW>
LH_DEV void store_px(float *p, const float (&v)[VW])
{
    if constexpr (VW == 4) {
        const lh_v4f t = {v[0], v[1], v[2], v[3]};
        __builtin_nontemporal_store(t, reinterpret_cast<lh_v4f *>(p));
    } else {
        const lh_v2f t = {v[0], v[1]};
        __builtin_nontemporal_store(t, reinterpret_cast<lh_v2f *>(p));
    }
}

LH_DEV void tile_coords(int t, const FrameGeom &g, int &f, int &bx, int &by)
{
    int r;
    if (g.interleave) {   // (kernel argument: uniform; all of this is scalar arithmetic)
        r = t / g.nframes;
        f = t - r * g.nframes;
    } else {
        f = t / g.tilesPerFrame;
        r = t - f * g.tilesPerFrame;
    }
    by = r / g.tilesX;
    bx = r - by * g.tilesX;
}

// ---- ENCODE ---------------------------------------------------------------------------------------
// CS: colour space; SUB: 4:2:0 (profiles 0/2) vs 4:4:4 (1/3); VW: pixels per thread per row (4 or 2);
// LM: luminance search mode (lut_index.hpp LutMode: 0 literal/LDS, 2 literal/global, 3 records/LDS, 4 records/global, 7 value-keyed records/LDS;
// 5 = YCbCr only: records in LDS for the composite luma -> code function, channel 0 carries the luma y, luma_device.hpp ycbcr_fwd;
// 6 = 5 + the half-input table in LDS: R', G', B' are three gathers for pixels whose inputs are binary16 values, luma_device.hpp half_lookup).
//
// Software pipeline: the six (VW=4: 16-byte) loads of the thread's NEXT unit are issued at the end of the current
// unit's iteration, one full iteration before they are needed (without this the kernel sat at ~45 % SQ_WAIT_ANY,
// profiles/r01_early_pmc_summary.txt); see the loop in k_encode for the order of loads and stores.

template <int VW>
struct EncUnit {
    float in[3][2][VW];
    int f, ux, uy;
    bool valid;
};

// IN16: the frames are binary16 (a.src[c] points at halves; offsets and strides count elements either way)
template <int VW, bool IN16 = false>
LH_DEV void enc_load(EncUnit<VW> &u, const EncArgs &a, int t, int tx, int ty, int NW)
{
    u.valid = false;
    if (t >= a.g.totalTiles)
        return;
    int bx, by;
    tile_coords(t, a.g, u.f, bx, by);
    u.ux = bx * 64 + tx;
    u.uy = by * NW + ty;
    if (u.ux >= a.g.unitsX || u.uy >= a.g.unitsY)
        return;
    u.valid = true;
    const size_t off = (size_t)u.f * a.frame_stride + (size_t)(2 * u.uy) * a.g.w + (size_t)u.ux * VW;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        if constexpr (IN16) {
            const _Float16 *hp = reinterpret_cast<const _Float16 *>(a.src[c]);
            load_px_h<VW>(hp + off, u.in[c][0]);
            load_px_h<VW>(hp + off + a.g.w, u.in[c][1]);
        } else {
            load_px<VW>(a.src[c] + off, u.in[c][0]);
            load_px<VW>(a.src[c] + off + a.g.w, u.in[c][1]);
        }
    }
}

struct EncStats {   // "no frame yet, nothing seen": what stats_flush leaves behind, too
    float sum = 0.0f, mn = __builtin_inff(), mx = -__builtin_inff();
    int frame = -1;
};

// Per-frame statistics: every wave adds its partial {sum, min, max} with three atomics.  Thousands of waves on ONE triple
// serialise at the L2 (a single 4K frame: 8192 waves, and the float min / max of the HIP headers are compare-and-swap loops
// -- the kernel took 1.08 ms instead of 30 us, profiles/r03_hostfed_trace.txt), so the arrivals are spread over STATS_SLOTS
// triples per frame (slot = workgroup index mod STATS_SLOTS) which k_fold_stats folds afterwards, and min / max use the
// hardware's integer atomics on the float's bit pattern: for v >= 0 the signed-integer order of the bits is the float order,
// for v < 0 the unsigned order is the reversed float order, and a negative float's bits exceed every non-negative one's as
// unsigned and undercut them as signed -- so min(v) = v >= 0 ? atomicMin(int) : atomicMax(unsigned), and the mirror image
// for max, are exact for any mix of signs starting from +inf / -inf.
constexpr int STATS_SLOTS = 32;

LH_DEV void atomic_min_f32(float *addr, float v)
{
    if (v >= 0.0f)
        atomicMin(reinterpret_cast<int *>(addr), __float_as_int(v));
    else
        atomicMax(reinterpret_cast<unsigned *>(addr), __float_as_uint(v));
}
LH_DEV void atomic_max_f32(float *addr, float v)
{
    if (v >= 0.0f)
        atomicMax(reinterpret_cast<int *>(addr), __float_as_int(v));
    else
        atomicMin(reinterpret_cast<unsigned *>(addr), __float_as_uint(v));
}

LH_DEV void stats_flush(EncStats &st, float *stats, int tx)
{
    if (st.frame >= 0) {
        const float s = wave_sum(st.sum), mn = wave_min(st.mn), mx = wave_max(st.mx);
        if (tx == 0) {
            float *p = stats + 3 * ((size_t)st.frame * STATS_SLOTS + (blockIdx.x & (STATS_SLOTS - 1)));
            atomicAdd(p + 0, s);
            if (mn == mn)   // (an all-NaN wave leaves +inf / -inf untouched, as fminf / fmaxf did within the wave)
                atomic_min_f32(p + 1, mn);
            if (mx == mx)
                atomic_max_f32(p + 2, mx);
        }
    }
    st.sum = 0.0f;
    st.mn = __builtin_inff();
    st.mx = -__builtin_inff();
}

// colour transform of one unit (row-major pixel order inside the unit: j = r*VW + i)
// HALF (YCbCr, LM == 6): the pixels go through the half-input table at `s_half` (LDS), which has `* sc` folded in
// Returns (HALF only) whether this thread's unit fell back to the general functions.
// STATS = false: the caller accumulates the statistics itself (k_transcode with the composite records, whose channel 0 is not the luminance)
template <int CS, int VW, bool YCODE = false, bool HALF = false, bool STATS = true, typename K>
LH_DEV bool enc_transform(EncUnit<VW> &u, const EncArgs &a, const K &k, float (&c0)[2 * VW],
                          float (&c1)[2 * VW], float (&c2)[2 * VW], EncStats &st, const float *s_half = nullptr)
{
    bool general = false;
    if (!HALF && k.sc != 1.0f) {  // wave-uniform; x*1.0f == x, so the multiply is skipped for the default preScaling
#pragma unroll
        for (int c = 0; c < 3; c++)
#pragma unroll
            for (int r = 0; r < 2; r++)
#pragma unroll
                for (int i = 0; i < VW; i++)
                    u.in[c][r][i] *= k.sc;
    }
    if constexpr (CS == CS_YCBCR) {
        float r8[2 * VW], g8[2 * VW], b8[2 * VW];
#pragma unroll
        for (int r = 0; r < 2; r++)
#pragma unroll
            for (int i = 0; i < VW; i++) {
                r8[r * VW + i] = u.in[0][r][i];
                g8[r * VW + i] = u.in[1][r][i];
                b8[r * VW + i] = u.in[2][r][i];
            }
        if constexpr (HALF)
            general = ycbcr_fwd_half_n<2 * VW>(r8, g8, b8, k, s_half, c0, c1, c2);
        else
            ycbcr_fwd_n<2 * VW, YCODE>(r8, g8, b8, k, c0, c1, c2);  // one "redo with the complete powf" decision per unit
    } else {
#pragma unroll
        for (int r = 0; r < 2; r++)
#pragma unroll
            for (int i = 0; i < VW; i++)
                xform_fwd<CS>(u.in[0][r][i], u.in[1][r][i], u.in[2][r][i], k, c0[r * VW + i], c1[r * VW + i], c2[r * VW + i]);
    }

    if (STATS && a.stats) {
#pragma unroll
        for (int j = 0; j < 2 * VW; j++) {
            st.sum += c0[j];
            st.mn = fminf(st.mn, c0[j]);
            st.mx = fmaxf(st.mx, c0[j]);
        }
    }
    return general;
}

// The codes of one transformed unit: quantize + subsample, stated once for every kernel that needs them.  Each row of codes is
// handed to `out` the moment it exists -- out.template row<N>(pl, r, codes): the N codes of plane pl that sit in row r of the
// unit (r = 0 for 4:2:0 chroma, whose unit is one row of VW / 2 samples) -- so a consumer that stores (EncStoreUnit, below) keeps
// plane 0 one row (VW searches in flight) at a time: that keeps the live register set small enough for 6 waves per SIMD.
template <int CS, bool SUB, int VW, int LM, typename LutPtr, typename IdxPtr, typename Out>
LH_DEV void enc_codes(const float (&c0)[2 * VW], const float (&c1)[2 * VW], const float (&c2)[2 * VW], const QuantDev &q, LutPtr lut, IdxPtr idx,
                      Out &out)
{
    constexpr bool LUT_ALL = (CS == CS_RGB || CS == CS_XYZ);  // planes 1,2 also go through the LUT
    const float maxC = q.maxC;
    // plane 0
#pragma unroll
    for (int r = 0; r < 2; r++) {
        float v[VW];
        int row[VW];
#pragma unroll
        for (int i = 0; i < VW; i++)
            v[i] = c0[r * VW + i];
        quantize_lut<LM, VW, CS == CS_LUV>(v, row, lut, idx, q);  // Lu'v': Y is >= 1e-4 or NaN
        out.template row<VW>(0, r, row);
    }

    // planes 1, 2
    if constexpr (SUB) {
        constexpr int NQ = VW / 2;
        float a1[NQ], a2[NQ];
#pragma unroll
        for (int qd = 0; qd < NQ; qd++) {
            // src/luma_encoder.cpp:287-289: 0.25f*(src[i] + src[i+1] + src[i+2w] + src[i+2w+1]); the factor is applied
            // below (LUT_ALL) or folded into the colour quantizer's scale (quantize_color_sum4)
            a1[qd] = ((c1[2 * qd] + c1[2 * qd + 1]) + c1[VW + 2 * qd]) + c1[VW + 2 * qd + 1];
            a2[qd] = ((c2[2 * qd] + c2[2 * qd + 1]) + c2[VW + 2 * qd]) + c2[VW + 2 * qd + 1];
        }
        int k1[NQ], k2[NQ];
        if constexpr (LUT_ALL) {
#pragma unroll
            for (int qd = 0; qd < NQ; qd++) {
                a1[qd] *= 0.25f;
                a2[qd] *= 0.25f;
            }
            quantize_lut<LM, NQ>(a1, k1, lut, idx, q);
            quantize_lut<LM, NQ>(a2, k2, lut, idx, q);
        } else {
            const float qc = 0.25f * maxC;
#pragma unroll
            for (int qd = 0; qd < NQ; qd++) {
                // Lu'v' chroma is positive or NaN (xform_fwd<CS_LUV>), so is the sum of four
                k1[qd] = quantize_color_sum4<CS == CS_LUV>(a1[qd], maxC, qc);
                k2[qd] = quantize_color_sum4<CS == CS_LUV>(a2[qd], maxC, qc);
            }
        }
        out.template row<NQ>(1, 0, k1);
        out.template row<NQ>(2, 0, k2);
    } else {
        int k1[2 * VW], k2[2 * VW];
        if constexpr (LUT_ALL) {
            quantize_lut<LM, 2 * VW>(c1, k1, lut, idx, q);
            quantize_lut<LM, 2 * VW>(c2, k2, lut, idx, q);
        } else {
#pragma unroll
            for (int j = 0; j < 2 * VW; j++) {
                k1[j] = quantize_color<CS == CS_LUV>(c1[j], maxC);
                k2[j] = quantize_color<CS == CS_LUV>(c2[j], maxC);
            }
        }
#pragma unroll
        for (int pl = 1; pl < 3; pl++) {
            int row[VW];
#pragma unroll
            for (int r = 0; r < 2; r++) {
#pragma unroll
                for (int i = 0; i < VW; i++)
                    row[i] = (pl == 1) ? k1[r * VW + i] : k2[r * VW + i];
                out.template row<VW>(pl, r, row);
            }
        }
    }
}

// "store a unit": pack the rows enc_codes hands over into unit (ux, uy) of frame f of the planes of `a`
template <bool SUB>
struct EncStoreUnit {
    const EncArgs &a;
    int f, ux, uy;
    template <int N>
    LH_DEVS void row(int pl, int r, const int (&codes)[N]) const
    {
        const int y0 = (SUB && pl) ? uy : 2 * uy;   // first plane row of the unit
        unsigned char *d = a.dst[pl] + (size_t)f * a.dst_frame_stride[pl] + (size_t)y0 * a.stride[pl] + (size_t)ux * N * a.bps;
        store_samples<N>(d + (size_t)r * a.stride[pl], codes, a.bps, a.aligned);
    }
};

// quantize + subsample + pack + store one transformed unit
template <int CS, bool SUB, int VW, int LM, typename LutPtr, typename IdxPtr>
LH_DEV void enc_emit(int f, int ux, int uy, const float (&c0)[2 * VW], const float (&c1)[2 * VW],
                     const float (&c2)[2 * VW], const EncArgs &a, LutPtr lut, IdxPtr idx)
{
    const EncStoreUnit<SUB> out{a, f, ux, uy};
    enc_codes<CS, SUB, VW, LM>(c0, c1, c2, a.q, lut, idx, out);
}

// ---- THE KERNELS THAT END IN enc_codes ----------------------------------------------------------------
// Two front ends produce a transformed unit (c0, c1, c2), three consumers take the codes enc_codes makes of it; the one that measures
// differences sums per frame (DistAcc, dist_flush) or per block (DistBlockAcc, dist_map_flush), the one that measures moments per
// block only (MomentBlockAcc, the same dist_map_flush):
//                                                        store (EncStoreUnit)   measure (DistMeasureUnit)   ... per block                 moments per block (MomentMeasureUnit)
//   frames in       FrameFront; enc_load, enc_transform  k_encode               k_distortion                k_distortion_map              k_moments_map
//   code planes in  PlaneFront; dec_load, dec_values,    k_transcode            k_transcode_distortion      k_transcode_distortion_map    k_transcode_moments_map
//                   enc_transform
//   code planes in, as they are: dec_issue, planes_rows  --                     k_planes_distortion         k_planes_distortion_map       k_planes_moments_map
//                   (no enc_codes: the planes' own samples are handed to the consumer in its order)
// A kernel is its front end, its consumer and the persistent loop that orders their loads against each other; the loops differ on
// purpose (stores before the next loads / the given words travelling along, one flush site) and stay written out.  Also written
// out: the stage_tables calls and, in the plane-fed kernels, the LDS pointers, kd / ke and the per-unit dec_values / enc_transform
// block -- behind a constructor or a helper they compile to other register allocations.

// The tables of the frame front end for colour space CS and search mode LM (stage_tables' WHAT)
template <int CS, int LM>
constexpr int frame_front_what()
{
    return (LM == 0 ? STAGE_LUT : 0) | ((LM == 3 || LM == 5 || LM == 6 || LM == 7) ? STAGE_REC : 0) |
           (CS == CS_YCBCR ? (LM == 6 ? STAGE_POWFN | STAGE_HALF : STAGE_POWF) : 0);
}

// Frames in: where stage_tables<WHAT>(smem, a.q, a.half) has put the tables of (CS, LM), and the constants enc_transform takes.
// LM == 6 (HALF): the 768-byte powf tables, the LDS belongs to the half-input table at s_half
template <int CS, int LM>
struct FrameFront {
    static_assert((LM != 5 && LM != 6) || CS == CS_YCBCR, "the composite records belong to the YCbCr kernels");
    static constexpr bool HALF = (LM == 6);
    static constexpr int WHAT = frame_front_what<CS, LM>();
    using PowTab = typename std::conditional<HALF, PowfTables, PowfTablesWide>::type;
    const float *s_lut;      // LM == 0
    const uint32_t *s_rec;   // LM == 3, 5, 6, 7
    const float *s_half;     // LM == 6
    XformConstT<PowTab> k;
    LH_DEVS FrameFront(unsigned char *smem, const EncArgs &a)
        : s_lut(reinterpret_cast<const float *>(smem + lds_table_offset<WHAT>())),
          s_rec(reinterpret_cast<const uint32_t *>(smem + lds_table_offset<WHAT>())),
          s_half(reinterpret_cast<const float *>(smem + lds_table_offset<WHAT>() + lds_rec_bytes(a.q))),
          k(make_xform_const<CS, PowTab>(a.sc, a.q.Lmax, reinterpret_cast<const PowTab *>(smem))) {}
};

// k_encode: every search mode (LM 0, 2, 4 too: the table or the records in global memory) and, with the half-input table, the
// workgroup's vote on whether the frames hold binary16 values
template <int CS, bool SUB, int VW, int LM, bool IN16 = false>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(EncWaves<CS, SUB, VW>::value))) void k_encode(const EncArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr bool HALF = (LM == 6);
    __shared__ int s_votes[HALF ? 2 : 1];   // HALF: waves of this workgroup that had units / that left the table in every one
    if (HALF && threadIdx.x == 0)
        s_votes[0] = s_votes[HALF ? 1 : 0] = 0;   // (stage_tables synchronises)
    stage_tables<FrameFront<CS, LM>::WHAT>(smem, a.q, a.half);
    const FrameFront<CS, LM> fr(smem, a);

    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int NW = blockDim.x >> 6;
    const int G = gridDim.x;

    EncStats st;

    // Per unit: transform, search / pack / store, THEN issue the next unit's loads (the current inputs are dead by then,
    // so both units share one set of registers); the other waves of the SIMD cover the load latency.  Issuing the loads
    // before the stores (round 1) measured 1.0-1.3 % slower HBM-fed, same-box, 5 of 5 interleaved rounds: with the
    // stores first the write bursts of a wave are not queued behind its own 6 KiB of reads.
    EncUnit<VW> u;
    int n_units = 0, n_general = 0;   // HALF: this wave's units, and those in which some lane left the table (wave-uniform)
    enc_load<VW, IN16>(u, a, blockIdx.x, tx, ty, NW);
    for (int t = blockIdx.x; t < a.g.totalTiles; t += G) {
        if (a.stats) {
            const int f = t / a.g.tilesPerFrame;  // wave-uniform
            if (f != st.frame) {
                stats_flush(st, a.stats, tx);
                st.frame = f;
            }
        }
        const bool valid = u.valid;
        const int f = u.f, ux = u.ux, uy = u.uy;
        float c0[2 * VW], c1[2 * VW], c2[2 * VW];
        bool general = false;
        if (valid)
            general = enc_transform<CS, VW, LM == 5 || LM == 6, HALF>(u, a, fr.k, c0, c1, c2, st, fr.s_half);
        if constexpr (HALF) {
            // a tile that overhangs the frame may leave this wave without a single pixel: such a unit is no evidence either way
            n_units += __builtin_amdgcn_ballot_w64(valid) != 0;
            n_general += __builtin_amdgcn_ballot_w64(general) != 0;
        }
        if (valid) {
            if constexpr (LM == 6)
                enc_emit<CS, SUB, VW, 5>(f, ux, uy, c0, c1, c2, a, fr.s_lut, fr.s_rec);
            else if constexpr (LM == 3 || LM == 5 || LM == 7)
                enc_emit<CS, SUB, VW, LM>(f, ux, uy, c0, c1, c2, a, fr.s_lut, fr.s_rec);
            else if constexpr (LM == 4)
                enc_emit<CS, SUB, VW, LM>(f, ux, uy, c0, c1, c2, a, a.q.lut, a.q.rec);
            else if constexpr (LM == 0)
                enc_emit<CS, SUB, VW, LM>(f, ux, uy, c0, c1, c2, a, fr.s_lut, fr.s_rec);
            else
                enc_emit<CS, SUB, VW, LM>(f, ux, uy, c0, c1, c2, a, a.q.lut, fr.s_rec);
        }
        enc_load<VW, IN16>(u, a, t + G, tx, ty, NW);
    }
    if (a.stats)
        stats_flush(st, a.stats, tx);
    if constexpr (HALF) {
        // Feedback: this workgroup reports "not binary16 data" when EVERY unit of EVERY one of its waves had a lane on the
        // general path -- with 1 % of the pixels off the table that is nearly every workgroup (and the table kernel then costs
        // 1.4 x the per-pixel one), with 0.1 % (where the table still wins) a wave sees such a unit 40 % of the time and
        // sixteen waves in a row essentially never do.
        if (a.half_flag) {   // (kernel argument: uniform)
            if (tx == 0 && n_units > 0) {
                atomicAdd(&s_votes[0], 1);
                if (n_general == n_units)
                    atomicAdd(&s_votes[1], 1);
            }
            __syncthreads();
            if (threadIdx.x == 0 && s_votes[0] > 0 && s_votes[0] == s_votes[1])
                __hip_atomic_store(a.half_flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// ---- DECODE ---------------------------------------------------------------------------------------
// GL: LUT read from global memory (bitdepth > 12) instead of LDS.  Same software pipeline as encode: the
// sample loads of the next unit are issued one iteration ahead, after the current unit's stores.
template <bool SUB, int VW>
struct DecUnit {
    int y[2][VW];
    int c1[SUB ? VW / 2 : 2 * VW];
    int c2[SUB ? VW / 2 : 2 * VW];
    int f, ux, uy;
    bool valid;
};

// Where row r of plane pl of the unit (f, ux, uy) begins, n samples of that plane to a unit row: THE statement of where a code
// plane's samples live, for every function that reads one.  A unit is two luminance rows deep; SUB: and one row of either chroma
// plane.  (The plane row is computed inside the sum, behind the frame's offset, and not handed in: with it computed first the
// compiler orders instructions of some transcode kernels differently, profiles/plane_loads_codegen.txt.)
template <bool SUB>
LH_DEV const unsigned char *dec_row(const DecArgs &a, int pl, int f, int ux, int uy, int r, int n)
{
    const int rows = (SUB && pl) ? 1 : 2;   // plane rows to a unit
    return a.src[pl] + (size_t)f * a.src_frame_stride[pl] + (size_t)(rows * uy + r) * a.stride[pl] + (size_t)ux * n * a.bps;
}

// The unpacking loads of the unit at u.f, u.ux, u.uy, once for everyone: dec_load (which finds the unit from its tile), dec_load_at
// (which is given it) and dec_finish (for the rows its vector loads cannot take, aligned = 0)
template <bool SUB, int VW>
LH_DEV void dec_load_rows(DecUnit<SUB, VW> &u, const DecArgs &a)
{
    const int f = u.f, ux = u.ux, uy = u.uy;
    {
        const unsigned char *s = dec_row<SUB>(a, 0, f, ux, uy, 0, VW);
        load_samples<VW>(s, u.y[0], a.bps, a.aligned);
        load_samples<VW>(s + a.stride[0], u.y[1], a.bps, a.aligned);
    }
    if constexpr (SUB) {
        constexpr int NQ = VW / 2;
        load_samples<NQ>(dec_row<SUB>(a, 1, f, ux, uy, 0, NQ), u.c1, a.bps, a.aligned);
        load_samples<NQ>(dec_row<SUB>(a, 2, f, ux, uy, 0, NQ), u.c2, a.bps, a.aligned);
    } else {
#pragma unroll
        for (int r = 0; r < 2; r++) {
            int row[VW];
            load_samples<VW>(dec_row<SUB>(a, 1, f, ux, uy, r, VW), row, a.bps, a.aligned);
#pragma unroll
            for (int i = 0; i < VW; i++)
                u.c1[r * VW + i] = row[i];
            load_samples<VW>(dec_row<SUB>(a, 2, f, ux, uy, r, VW), row, a.bps, a.aligned);
#pragma unroll
            for (int i = 0; i < VW; i++)
                u.c2[r * VW + i] = row[i];
        }
    }
}

// The unit of lane (tx, ty) in tile t; u.valid: the tile exists and the unit lies inside the frame
template <bool SUB, int VW>
LH_DEV void dec_load(DecUnit<SUB, VW> &u, const DecArgs &a, int t, int tx, int ty, int NW)
{
    u.valid = false;
    if (t >= a.g.totalTiles)
        return;
    int bx, by;
    tile_coords(t, a.g, u.f, bx, by);
    u.ux = bx * 64 + tx;
    u.uy = by * NW + ty;
    if (u.ux >= a.g.unitsX || u.uy >= a.g.unitsY)
        return;
    u.valid = true;
    dec_load_rows<SUB, VW>(u, a);
}

// The unit at given coordinates: no tile arithmetic and no range test, both the caller's (k_transcode_half, whose loop runs over
// the target's tiles and whose source units are in range whenever the target unit is).  The unit records its coordinates as
// dec_load's does, so that a DecUnit is one thing wherever it was loaded; k_transcode_half itself reads only the samples.
template <bool SUB, int VW>
LH_DEV void dec_load_at(DecUnit<SUB, VW> &u, const DecArgs &a, int f, int ux, int uy)
{
    u.valid = true;
    u.f = f;
    u.ux = ux;
    u.uy = uy;
    dec_load_rows<SUB, VW>(u, a);
}

// ---- the same loads as a REAL prefetch (round 6) ---------------------------------------------------------------------
// dec_load unpacks every row right behind its load, so the compiler has to wait for each load (s_waitcnt vmcnt(0): the unit's
// four loads are four serial round trips, each also waiting for every store issued before it) -- harmless where twenty waves per
// CU hide it, but the YCbCr kernels run four waves per SIMD with microseconds of arithmetic per unit and spent most of a unit's
// time in those waits.  DecRaw keeps the rows as loaded (six registers for 4:2:0 16-bit); dec_issue issues the loads of the NEXT
// unit before the current unit is processed, and dec_finish unpacks them after the current unit's arithmetic and BEFORE its
// stores (dec_process's hook): the one wait of an iteration then sits where only those loads and the previous unit's stores --
// a whole unit's arithmetic old -- are outstanding, and this unit's stores are not waited for until the next one's arithmetic
// is done.  (The compiler's waits are vmcnt(0) throughout: one counter for loads and stores on gfx950, and the conditional
// stores of the loop defeat exact counting.)  Rows the vector loads cannot take (a.aligned == 0: odd strides of a
// lossy upstream decoder) are loaded by dec_finish as dec_load does.
template <bool SUB, int VW>
struct DecRaw {
    uint32_t y[2][2];
    uint32_t c1[SUB ? 1 : 2][2], c2[SUB ? 1 : 2][2];
    int f, ux, uy;
    bool valid;
};

template <int N>
LH_DEV void load_raw(const unsigned char *p, uint32_t (&r)[2], int bps)
{
    const int bytes = N * bps;   // 8, 4, 2 or 1; uniform
    if (bytes == 8) {
        const lh_v2u v = __builtin_nontemporal_load(reinterpret_cast<const lh_v2u *>(p));
        r[0] = v.x;
        r[1] = v.y;
    } else if (bytes == 4) {
        r[0] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t *>(p));
    } else if (bytes == 2) {
        r[0] = __builtin_nontemporal_load(reinterpret_cast<const uint16_t *>(p));
    } else {
        r[0] = p[0];
    }
}

template <int N>
LH_DEV void unpack_raw(const uint32_t (&r)[2], int (&c)[N], int bps)
{
    if (bps == 2) {
        if constexpr (N == 4) {
            c[0] = r[0] & 0xffff; c[1] = r[0] >> 16; c[2] = r[1] & 0xffff; c[3] = r[1] >> 16;
        } else if constexpr (N == 2) {
            c[0] = r[0] & 0xffff; c[1] = r[0] >> 16;
        } else {
            c[0] = r[0] & 0xffff;
        }
    } else {
        if constexpr (N == 4) {
            c[0] = r[0] & 0xff; c[1] = (r[0] >> 8) & 0xff; c[2] = (r[0] >> 16) & 0xff; c[3] = r[0] >> 24;
        } else if constexpr (N == 2) {
            c[0] = r[0] & 0xff; c[1] = (r[0] >> 8) & 0xff;
        } else {
            c[0] = r[0] & 0xff;
        }
    }
}

template <bool SUB, int VW>
LH_DEV void dec_issue(DecRaw<SUB, VW> &u, const DecArgs &a, int t, int tx, int ty, int NW)
{
    // (dec_load's tile -> unit lines, written out a second time: behind a function shared with dec_load -- returning bool, or void
    //  with the test on u.valid -- every kernel that calls dec_issue compiles to other instructions, profiles/plane_loads_codegen.txt)
    u.valid = false;
    if (t >= a.g.totalTiles)
        return;
    int bx, by;
    tile_coords(t, a.g, u.f, bx, by);
    u.ux = bx * 64 + tx;
    u.uy = by * NW + ty;
    if (u.ux >= a.g.unitsX || u.uy >= a.g.unitsY)
        return;
    u.valid = true;
    if (!a.aligned)
        return;   // (dec_finish loads these rows itself)
    const int f = u.f, ux = u.ux, uy = u.uy;
    const unsigned char *s = dec_row<SUB>(a, 0, f, ux, uy, 0, VW);
    load_raw<VW>(s, u.y[0], a.bps);
    load_raw<VW>(s + a.stride[0], u.y[1], a.bps);
    if constexpr (SUB) {
        constexpr int NQ = VW / 2;
        load_raw<NQ>(dec_row<SUB>(a, 1, f, ux, uy, 0, NQ), u.c1[0], a.bps);
        load_raw<NQ>(dec_row<SUB>(a, 2, f, ux, uy, 0, NQ), u.c2[0], a.bps);
    } else {
#pragma unroll
        for (int r = 0; r < 2; r++) {
            load_raw<VW>(dec_row<SUB>(a, 1, f, ux, uy, r, VW), u.c1[r], a.bps);
            load_raw<VW>(dec_row<SUB>(a, 2, f, ux, uy, r, VW), u.c2[r], a.bps);
        }
    }
}

template <bool SUB, int VW>
LH_DEV void dec_finish(DecUnit<SUB, VW> &u, const DecRaw<SUB, VW> &w, const DecArgs &a)
{
    u.f = w.f;
    u.ux = w.ux;
    u.uy = w.uy;
    u.valid = w.valid;
    if (!w.valid)
        return;
    if (a.aligned) {
        unpack_raw<VW>(w.y[0], u.y[0], a.bps);
        unpack_raw<VW>(w.y[1], u.y[1], a.bps);
        if constexpr (SUB) {
            unpack_raw<VW / 2>(w.c1[0], u.c1, a.bps);
            unpack_raw<VW / 2>(w.c2[0], u.c2, a.bps);
        } else {
#pragma unroll
            for (int r = 0; r < 2; r++) {
                int row[VW];
                unpack_raw<VW>(w.c1[r], row, a.bps);
#pragma unroll
                for (int i = 0; i < VW; i++)
                    u.c1[r * VW + i] = row[i];
                unpack_raw<VW>(w.c2[r], row, a.bps);
#pragma unroll
                for (int i = 0; i < VW; i++)
                    u.c2[r * VW + i] = row[i];
            }
        }
        return;
    }
    dec_load_rows<SUB, VW>(u, a);   // (a.aligned is 0 here)
}

// the unit's samples must be in registers HERE (the compiler may not sink the unpacking, and with it the wait for the loads,
// below the stores that follow)
template <bool SUB, int VW>
LH_DEV void dec_pin(DecUnit<SUB, VW> &u)
{
#pragma unroll
    for (int r = 0; r < 2; r++)
#pragma unroll
        for (int i = 0; i < VW; i++)
            asm volatile("" : "+v"(u.y[r][i]));
#pragma unroll
    for (int j = 0; j < (SUB ? VW / 2 : 2 * VW); j++) {
        asm volatile("" : "+v"(u.c1[j]));
        asm volatile("" : "+v"(u.c2[j]));
    }
}

// Whether this wave reads red and blue of the current unit from the per-stream tables (k_decode<..., RB>) or computes them.
// What a gather costs is decided by the CU's 32 KiB vector L1 (profiles/r05_ycbcr_decode_tables.txt, TCP_TCC_READ_REQ): a
// table line holds 32 consecutive luminance codes of ONE colour code; with the codes of a picture a lane's eight pixels read
// two lines per table, its neighbours and the rows above and below read the same ones, 99 % of the lanes hit the L1 and the
// launch takes 0.80 ms per 20 x 4K against 1.23 for six powf per pixel.  With unrelated codes in every pixel (the synthetic
// stream of SURVEY 8(d)) every lane of every gather is its own L2 request -- 3.2e8 per launch, the L2's request rate -- and the
// same launch takes 1.84 ms.  So a wave looks at its codes first, per unit, wave-uniformly (no divergence), ~20 instructions:
// a lane is "local" when its eight luminance codes lie within `near_y` of each other, its first luminance code within near_y
// of its left neighbour lane's, and its first colour codes within near_c (|dCb| + |dCr|) of that neighbour's; the wave gathers
// when at least RB_LOCAL_LANES of its lanes are.  Whichever path runs, the results are the same bits.
constexpr int RB_LOCAL_LANES = 48;

LH_DEV uint32_t sad_u32(uint32_t a, uint32_t b, uint32_t acc)
{
    uint32_t r;
    asm("v_sad_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(acc));   // |a - b| + acc
    return r;
}

// the value of lane - 1 (lane 0: 0)
LH_DEV uint32_t left_lane(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false); }

template <bool SUB, int VW>
LH_DEV bool rb_wave_local(const DecUnit<SUB, VW> &u, int near_y, int near_c)
{
    if (near_y < 0)
        return true;
    int lo = u.y[0][0], hi = u.y[0][0];
#pragma unroll
    for (int r = 0; r < 2; r++)
#pragma unroll
        for (int i = 0; i < VW; i++) {
            lo = min(lo, u.y[r][i]);
            hi = max(hi, u.y[r][i]);
        }
    const uint32_t y0 = (uint32_t)u.y[0][0], b0 = (uint32_t)u.c1[0], r0 = (uint32_t)u.c2[0];
    const uint32_t dy = sad_u32(y0, left_lane(y0), 0u);
    const uint32_t dc = sad_u32(r0, left_lane(r0), sad_u32(b0, left_lane(b0), 0u));
    const bool local = (hi - lo) <= near_y && dy <= (uint32_t)near_y && dc <= (uint32_t)near_c;
    return __builtin_popcountll(__builtin_amdgcn_ballot_w64(local)) >= RB_LOCAL_LANES;
}

// SCFAST (YCbCr): the straight-line code divides by sc with the short division (XformConst::sc_mode == 1, ycbcr_inv_n)
// Returns (RB only; wave-uniform) whether the wave took red and blue of this unit from the tables.
// before_stores: called once between the unit's arithmetic and its stores (the prefetching loop of k_decode completes the NEXT
// unit's loads there)
struct DecNoHook {
    __device__ __forceinline__ void operator()() const {}
};
// OUT16: the frames are binary16 (a.dst[c] points at halves; offsets and strides count elements either way)
// VALUES: nothing is stored; the unit's floats -- after `/ sc`: what the reference stores in its LumaFrame -- go to vals[c][r][i],
// colour channel c of pixel i in row r (dec_values below, for k_transcode)
template <int CS, bool SUB, int VW, bool DISP, bool UVTAB, bool YT = false, bool SCFAST = false, bool RB = false, bool OUT16 = false, bool VALUES = false,
          typename LutPtr, typename K, typename Hook = DecNoHook>
LH_DEV bool dec_process(const DecUnit<SUB, VW> &u, const DecArgs &a, const K &k, LutPtr lut, const float *s_uv, Hook before_stores = Hook(),
                        float (*vals)[2][VW] = nullptr)
{
    bool gathered = false;
    static_assert(!RB || (YT && CS == CS_YCBCR), "the red / blue tables belong to the YCbCr kernels with the y table");
    constexpr bool LUT_ALL = (CS == CS_RGB || CS == CS_XYZ);
    const float maxC = a.q.maxC;
    const int maxVal = a.q.maxVal;
    float c0[2 * VW], c1[2 * VW], c2[2 * VW];
#pragma unroll
    for (int r = 0; r < 2; r++)
#pragma unroll
        for (int i = 0; i < VW; i++)
            c0[r * VW + i] = dequantize_lut(u.y[r][i], YT ? LutPtr(s_uv) : lut, maxVal);   // YT: the y table (behind the table in LDS)
    if constexpr (CS == CS_YCBCR && YT) {
        // (the chroma samples are read as terms from the per-code tables below)
    } else if constexpr (SUB) {
        constexpr int NQ = VW / 2;
#pragma unroll
        for (int qd = 0; qd < NQ; qd++) {
            const float v1 = LUT_ALL ? dequantize_lut(u.c1[qd], lut, maxVal) : dequantize_color(u.c1[qd], maxC);
            const float v2 = LUT_ALL ? dequantize_lut(u.c2[qd], lut, maxVal) : dequantize_color(u.c2[qd], maxC);
            // src/luma_decoder.cpp:229-234: the sample is replicated to its 2x2 block
            c1[2 * qd] = c1[2 * qd + 1] = c1[VW + 2 * qd] = c1[VW + 2 * qd + 1] = v1;
            c2[2 * qd] = c2[2 * qd + 1] = c2[VW + 2 * qd] = c2[VW + 2 * qd + 1] = v2;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 2 * VW; j++) {
            c1[j] = LUT_ALL ? dequantize_lut(u.c1[j], lut, maxVal) : dequantize_color(u.c1[j], maxC);
            c2[j] = LUT_ALL ? dequantize_lut(u.c2[j], lut, maxVal) : dequantize_color(u.c2[j], maxC);
        }
    }
    float out[3][2][VW];
    if constexpr (CS == CS_LUV) {
        // chroma-only factors once per quad (4:2:0) / per pixel (4:4:4), on the short division path when the
        // codes are in range (always, unless a lossy upstream decoder produced garbage)
        constexpr int NC = SUB ? VW / 2 : 2 * VW;
        const int maxCi = (int)maxC;
        const float rmaxC = rcp_nr(maxC);
        LuvChroma ch[NC];
#pragma unroll
        for (int j = 0; j < NC; j++) {
            if (u.c1[j] <= maxCi && u.c2[j] <= maxCi) {
                if constexpr (UVTAB)
                    ch[j] = luv_chroma_uv(s_uv[u.c1[j]], s_uv[u.c2[j]]);
                else
                    ch[j] = luv_chroma<true>(dequantize_color_safe(u.c1[j], maxC, rmaxC), dequantize_color_safe(u.c2[j], maxC, rmaxC));
            } else {
                ch[j] = luv_chroma<false>(dequantize_color(u.c1[j], maxC), dequantize_color(u.c2[j], maxC));
            }
        }
#pragma unroll
        for (int r = 0; r < 2; r++)
#pragma unroll
            for (int i = 0; i < VW; i++)
                luv_apply(c0[r * VW + i], ch[SUB ? i / 2 : r * VW + i], out[0][r][i], out[1][r][i], out[2][r][i]);
    } else if constexpr (CS == CS_YCBCR) {
        float r8[2 * VW], g8[2 * VW], b8[2 * VW];
        if constexpr (YT) {
            // the chroma terms from the per-code tables behind the y table (stage_tables, STAGE_CT); the codes themselves go
            // along for the complete functions, which a code beyond maxC (garbage from a lossy upstream decoder) calls for
            constexpr int NC = SUB ? VW / 2 : 2 * VW;
            const int maxCi = (int)maxC;
            const float *s_cb = s_uv + (a.q.lut_len + a.q.pad), *s_cr = s_cb + (maxCi + 1);
            bool bad = false;
#pragma unroll
            for (int j = 0; j < NC; j++) {
                bad = bad || u.c1[j] > maxCi || u.c2[j] > maxCi;
                const float t1 = s_cb[min(u.c1[j], maxCi)], t2 = s_cr[min(u.c2[j], maxCi)];
                if constexpr (SUB) {
                    c1[2 * j] = c1[2 * j + 1] = c1[VW + 2 * j] = c1[VW + 2 * j + 1] = t1;
                    c2[2 * j] = c2[2 * j + 1] = c2[VW + 2 * j] = c2[VW + 2 * j + 1] = t2;
                } else {
                    c1[j] = t1;
                    c2[j] = t2;
                }
            }
            bool gather = false;
            if constexpr (RB)
                gather = rb_wave_local<SUB, VW>(u, a.rb_near_y, a.rb_near_c);   // wave-uniform
            gathered = gather;
            if (RB && gather) {
                // red and blue of every pixel from the per-stream tables: two 4-byte gathers from global memory, issued before
                // green's two powf chains (which cover their latency); plain loads -- these lines are worth caching
                float tr[2 * VW], tb[2 * VW];
                const size_t n = (size_t)a.q.lut_len;
#pragma unroll
                for (int r = 0; r < 2; r++)
#pragma unroll
                    for (int i = 0; i < VW; i++) {
                        const int j = SUB ? i / 2 : r * VW + i;
                        const size_t yc = (size_t)min(u.y[r][i], maxVal);
                        tb[r * VW + i] = a.rb[(size_t)min(u.c1[j], maxCi) * n + yc];
                        tr[r * VW + i] = a.rb[a.rb_plane + (size_t)min(u.c2[j], maxCi) * n + yc];
                    }
                const bool redo = ycbcr_inv_green_n<2 * VW, SCFAST ? 1 : 0, NC, SUB>(c0, c1, c2, k, r8, g8, b8, u.c1, u.c2, maxC, bad);
                if (!redo) {
#pragma unroll
                    for (int j = 0; j < 2 * VW; j++) {
                        r8[j] = tr[j];
                        b8[j] = tb[j];
                    }
                }
            } else {
                ycbcr_inv_n<2 * VW, true, SCFAST ? 1 : 0, true, NC, SUB>(c0, c1, c2, k, r8, g8, b8, u.c1, u.c2, maxC, bad);
            }
        } else {
            ycbcr_inv_n<2 * VW, YT, SCFAST ? 1 : 0>(c0, c1, c2, k, r8, g8, b8);
        }
#pragma unroll
        for (int r = 0; r < 2; r++)
#pragma unroll
            for (int i = 0; i < VW; i++) {
                out[0][r][i] = r8[r * VW + i];
                out[1][r][i] = g8[r * VW + i];
                out[2][r][i] = b8[r * VW + i];
            }
    } else {
#pragma unroll
        for (int r = 0; r < 2; r++)
#pragma unroll
            for (int i = 0; i < VW; i++)
                xform_inv<CS>(c0[r * VW + i], c1[r * VW + i], c2[r * VW + i], k, out[0][r][i], out[1][r][i], out[2][r][i]);
    }
    if (CS != CS_YCBCR && k.sc != 1.0f) {  // wave-uniform; x/1.0f == x, so the division is skipped for the default preScaling (YCbCr: ycbcr_inv_n has divided)
#pragma unroll
        for (int c = 0; c < 3; c++)
#pragma unroll
            for (int r = 0; r < 2; r++)
#pragma unroll
                for (int i = 0; i < VW; i++)
                    out[c][r][i] = div_ieee(out[c][r][i], k.sc);
    }

    if constexpr (VALUES) {
        static_assert(!DISP && !OUT16, "values only: no stores of any kind");
#pragma unroll
        for (int c = 0; c < 3; c++)
#pragma unroll
            for (int r = 0; r < 2; r++)
#pragma unroll
                for (int i = 0; i < VW; i++)
                    vals[c][r][i] = out[c][r][i];
        return gathered;
    }
    before_stores();
    if constexpr (OUT16) {
        // (packed and planar frames only: the host never sets rot_on for these kernels, lumahip_decode_frames_device_f16)
        static_assert(!DISP, "binary16 frames have no display epilogue");
        const size_t off = (size_t)u.f * a.frame_stride + (size_t)(2 * u.uy) * a.g.w + (size_t)u.ux * VW;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            uint16_t *d = reinterpret_cast<uint16_t *>(a.dst[c]) + off;
            store_px_h<VW>(d, out[c][0]);
            store_px_h<VW>(d + a.g.w, out[c][1]);
        }
    } else if (!DISP || a.dst[0]) {
        const size_t px = (size_t)(2 * u.uy) * a.g.w + (size_t)u.ux * VW;
        if (a.rot_on) {   // (kernel argument: uniform; u.f is wave-uniform, so the base is a scalar select)
            // (readfirstlane: the frame index IS wave-uniform, and saying so keeps the choice among the three bases a scalar one.
            //  Without it the compiler -- once `a` is reachable through the loop's lambdas -- reads a.rot[j] with a VECTOR load from
            //  the kernel arguments and waits for it with vmcnt(0) right in front of the stores, i.e. for every store of the
            //  previous unit: 0.744 -> 0.683 of the roofline on this path, found in two default bench runs.)
            const int fu = __builtin_amdgcn_readfirstlane(u.f);
            const int k = fu / 3, j = fu - 3 * k;
            float *base = (j == 0 ? a.rot[0] : j == 1 ? a.rot[1] : a.rot[2]) + (size_t)k * a.frame_stride + px;
            const size_t n1 = (size_t)a.g.w * a.g.h;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                store_px<VW>(base + c * n1, out[c][0]);
                store_px<VW>(base + c * n1 + a.g.w, out[c][1]);
            }
        } else {
            const size_t off = (size_t)u.f * a.frame_stride + px;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                store_px<VW>(a.dst[c] + off, out[c][0]);
                store_px<VW>(a.dst[c] + off + a.g.w, out[c][1]);
            }
        }
    }
    if constexpr (DISP) {
        // Display-side transform of the player (src/lumaplay_dequantizer.frag:145-156) on the decoded,
        // already /sc-scaled RGB: exposure, optional 8-bit LDR simulation, optional sigmoid tone curve,
        // display gamma, 8-bit UNORM.  Not bit-pinned by the reference (its LUT texture is GL_LINEAR filtered),
        // so the fast fp32 pow (v_exp(v_log)) is used here; tolerance +-1 code against a float64 evaluation.
#pragma unroll
        for (int r = 0; r < 2; r++) {
            uint32_t px[VW];
#pragma unroll
            for (int i = 0; i < VW; i++) {
                uint32_t packed = 0xff000000u;
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    float v = out[c][r][i];
                    if (a.ldr_sim)
                        v = a.exposure * fmaxf(1.0f, fminf(256.0f, floorf(256.0f * v))) * (1.0f / 256.0f);
                    else
                        v = v * a.exposure;
                    if (a.do_tmo) {
                        const float vn = __powf(fmaxf(v, 0.0f), 0.8f);
                        v = vn / (vn + 0.83650957f);  // pow(0.8, 0.8)
                    }
                    v = __powf(fmaxf(v, 0.0f), a.inv_gamma);
                    v = fminf(fmaxf(v, 0.0f), 1.0f);  // NaN -> 0
                    packed |= (uint32_t)(v * 255.0f + 0.5f) << (8 * c);
                }
                px[i] = packed;
            }
            unsigned char *d = a.disp + (size_t)u.f * a.disp_frame_stride + (size_t)(2 * u.uy + r) * a.disp_stride +
                               (size_t)u.ux * VW * 4;
#pragma unroll
            for (int i = 0; i < VW; i++)
                reinterpret_cast<uint32_t *>(d)[i] = px[i];
        }
    }
    return gathered;
}

// the arithmetic of dec_process alone: out = the unit's floats, in the layout of EncUnit::in
template <int CS, bool SUB, int VW, bool UVTAB, bool YT = false, bool SCFAST = false, typename LutPtr, typename K>
LH_DEV void dec_values(const DecUnit<SUB, VW> &u, const DecArgs &a, const K &k, LutPtr lut, const float *s_uv, float (&out)[3][2][VW])
{
    dec_process<CS, SUB, VW, false, UVTAB, YT, SCFAST, false, false, true>(u, a, k, lut, s_uv, DecNoHook(), out);
}

// DISP: additionally (or only) emit the RGBA8 display image -- a separate instantiation so that the plain
// decoder does not carry the epilogue's registers (it cost 8 % when it was a run-time branch)
// YT (YCbCr, table in LDS): additionally stage the per-stream y table and skip the first PQ evaluation of every pixel
// RB (with YT): red and blue from the per-stream (Y', Cr) / (Y', Cb) tables in global memory, green computed (DecArgs::rb)
// OUT16: binary16 frames (dec_process), packed or planar; never with DISP or the rotating layout
template <int CS, bool SUB, int VW, bool GL, bool DISP = false, bool YT = false, bool RB = false, bool OUT16 = false>
__global__ __launch_bounds__(1024) void k_decode(const DecArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    static_assert(!OUT16 || !DISP, "binary16 frames have no display epilogue");
    static_assert(!YT || (CS == CS_YCBCR && !GL), "the y table belongs to the YCbCr kernels with the table in LDS");
    static_assert(!RB || YT, "the red / blue tables need the y table");
    // GL: transfer-function table or chroma depth beyond 12 bits -- tables stay in global memory / are not built
    constexpr bool UVTAB = (CS == CS_LUV && !GL);
    // (The 16-entry powf tables instead -- no LDS bank conflicts, ten more issue cycles per powf -- were tried for this kernel
    // once the round-4 changes had cut its VALU work by 13 %: 3.3 % slower, 1.296 against 1.253 ms per 20 x 4K, same box.)
    using DecTab = PowfTablesWide;
    constexpr int WHAT = (GL ? 0 : STAGE_LUT) | (CS == CS_YCBCR ? STAGE_POWF : 0) | (UVTAB ? STAGE_UV : 0) | (YT ? STAGE_YT | STAGE_CT : 0);
    __shared__ int s_gathered[1];
    if (RB && threadIdx.x == 0)
        s_gathered[0] = 0;   // (before the barrier inside stage_tables: no wave can report ahead of the reset; the one reader
                             //  waits at the barrier at the end)
    stage_tables<WHAT>(smem, a.q);
    const float *s_lut = reinterpret_cast<const float *>(smem + lds_table_offset<WHAT>());
    const float *s_uv = reinterpret_cast<const float *>(smem + lds_table_offset<WHAT>() + lds_lut_bytes(a.q));
    const XformConstT<DecTab> k = make_xform_const<CS, DecTab>(a.sc, a.q.Lmax, reinterpret_cast<const DecTab *>(smem));

    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int NW = blockDim.x >> 6;
    const int G = gridDim.x;

    bool any_gather = false;
    // How the next unit's rows are loaded (same-box A/B per kernel family, profiles/r06_decode_prefetch.txt):
    //   PF   raw loads BEFORE this unit is processed, unpacked between its arithmetic and its stores (DecRaw above): the YCbCr
    //        kernels (-2.5 % on unrelated pixels, +5 % on pictures) and every 4:4:4 kernel (six row loads per unit that used to be
    //        six serial round trips: -10 ... -17 %);
    //   !PF  dec_load behind this unit's stores: the 4:2:0 kernels of the HBM-bound colour spaces, whose 16-bit samples (BASELINE's
    //        profile 2) are 4 - 6 % SLOWER with four loads in flight per wave instead of one round trip after another.
    // (The record also holds the rejected third form, raw loads after the stores: it helped only 8-bit 4:2:0.)
    // The loop stays inside this lambda, a leftover of the time it was instantiated per form: written straight into the kernel
    // nearly every k_decode compiles to other instructions (profiles/plane_loads_codegen.txt).
    auto run = [&](auto pf_tag) {
    constexpr bool PF = decltype(pf_tag)::value;
    DecUnit<SUB, VW> cur, nxt;
    DecRaw<SUB, VW> nxt_w;
    if constexpr (PF) {
        dec_issue<SUB, VW>(nxt_w, a, blockIdx.x, tx, ty, NW);
        dec_finish<SUB, VW>(cur, nxt_w, a);
    } else {
        dec_load<SUB, VW>(cur, a, blockIdx.x, tx, ty, NW);
    }
    for (int t = blockIdx.x; t < a.g.totalTiles; t += G) {
        if constexpr (PF)
            dec_issue<SUB, VW>(nxt_w, a, t + G, tx, ty, NW);
        auto hook = [&]() {
            if constexpr (PF) {
                dec_finish<SUB, VW>(nxt, nxt_w, a);
                if (nxt.valid)
                    dec_pin<SUB, VW>(nxt);
            }
        };
        if (cur.valid) {
            if constexpr (CS == CS_YCBCR) {
                // two copies of the unit's code, chosen by a kernel argument: see ycbcr_inv_n on why not a run-time choice inside
                if (k.sc_mode == 1) {
                    if constexpr (GL)
                        dec_process<CS, SUB, VW, DISP, false, false, true, false, OUT16>(cur, a, k, a.q.lut, s_uv, hook);
                    else
                        any_gather |= dec_process<CS, SUB, VW, DISP, UVTAB, YT, true, RB, OUT16>(cur, a, k, s_lut, s_uv, hook);
                } else {
                    if constexpr (GL)
                        dec_process<CS, SUB, VW, DISP, false, false, false, false, OUT16>(cur, a, k, a.q.lut, s_uv, hook);
                    else
                        any_gather |= dec_process<CS, SUB, VW, DISP, UVTAB, YT, false, RB, OUT16>(cur, a, k, s_lut, s_uv, hook);
                }
            } else if constexpr (GL) {
                dec_process<CS, SUB, VW, DISP, false, false, false, false, OUT16>(cur, a, k, a.q.lut, s_uv, hook);
            } else {
                dec_process<CS, SUB, VW, DISP, UVTAB, YT, false, false, OUT16>(cur, a, k, s_lut, s_uv, hook);
            }
        } else {
            hook();
        }
        if constexpr (!PF)
            dec_load<SUB, VW>(nxt, a, t + G, tx, ty, NW);
        cur = nxt;
    }
    };   // run
    run(std::integral_constant<bool, (CS == CS_YCBCR || !SUB)>());
    if constexpr (RB) {
        if (a.rb_flag) {   // (kernel argument: uniform)
            if (any_gather)
                s_gathered[0] = 1;   // (same value from every writer)
            __syncthreads();
            if (threadIdx.x == 0 && s_gathered[0])
                __hip_atomic_store(a.rb_flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// ---- TRANSCODE --------------------------------------------------------------------------------------
// Code planes of one stream -> code planes of another, DEC then ENC of the head of this file without the float frame between
// them: per unit, dec_load and dec_values under the source quantizer (`/ sc` of the source included), the floats handed to
// enc_transform in registers (`* sc` of the target included: the division and the multiplication both stay, the planes are the
// two-call result bit for bit), enc_codes under the target quantizer.  6 B per pixel instead of 30 (profile 2 -> profile 2).
// CSD / SUBD: the source's colour space and subsampling, CSE / SUBE: the target's -- independent; 4:4:4 -> 4:2:0 averages the
// per-pixel chroma as enc_codes does, 4:2:0 -> 4:4:4 stores the replicated sample's code four times.
// LM: the target's search mode: 3 or 7 (Lu'v': the luminance records in LDS), 5 (YCbCr: the composite records in LDS).
// Source side: the luminance table in LDS, plus the u'v' table (Lu'v') or the y table and the two chroma-term tables (YCbCr);
// red and blue are always computed (no per-stream red / blue tables, no feedback word: the launch is a function of the
// arguments alone).  LDS: [powf tables, once, when either side is YCbCr][source tables][target records] (stage_tables<A, B>).
struct TransArgs {
    DecArgs d;   // q, src, stride, src_frame_stride, sc, bps, aligned of the source planes; g (the same geometry as e.g)
    EncArgs e;   // q (the composite records for LM == 5), dst, stride, dst_frame_stride, sc, bps, aligned, stats of the target planes
};

// Code planes in: the supported pairs and what stage_tables<WHAT_D, WHAT_E> stages for the source's and the target's quantizer
template <int CSD, int CSE, int LM>
struct PlaneFront {
    static_assert(CSD == CS_LUV || CSD == CS_YCBCR, "source colour spaces: Lu'v' and YCbCr");
    static_assert((CSE == CS_LUV && (LM == 3 || LM == 7)) || (CSE == CS_YCBCR && LM == 5), "target: Lu'v' with records in LDS, YCbCr with the composite records");
    static constexpr bool YD = CSD == CS_YCBCR, YE = CSE == CS_YCBCR;
    static constexpr int WHAT_D = STAGE_LUT | (YD ? STAGE_POWF | STAGE_YT | STAGE_CT : STAGE_UV);
    static constexpr int WHAT_E = STAGE_REC | (YE ? STAGE_POWF : 0);
};

// k_transcode: the statistics of the target planes (a.e.stats), and k_encode's loop -- the next unit's sample loads are issued
// after the current unit's stores
template <int CSD, bool SUBD, int CSE, bool SUBE, int VW, int LM>
__global__ __launch_bounds__(1024) void k_transcode(const TransArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    using Front = PlaneFront<CSD, CSE, LM>;
    stage_tables<Front::WHAT_D, Front::WHAT_E>(smem, a.d.q, a.e.q);
    constexpr int off = lds_table_offset<Front::WHAT_D | Front::WHAT_E>();
    const float *s_lut = reinterpret_cast<const float *>(smem + off);
    const float *s_uv = reinterpret_cast<const float *>(smem + off + lds_lut_bytes(a.d.q));   // u'v' table, or y table + chroma terms
    const uint32_t *s_rec = reinterpret_cast<const uint32_t *>(smem + off + lds_quant_bytes<Front::WHAT_D>(a.d.q));
    const PowfTablesWide *pw = reinterpret_cast<const PowfTablesWide *>(smem);
    const XformConst kd = make_xform_const<CSD>(a.d.sc, a.d.q.Lmax, pw);
    const XformConst ke = make_xform_const<CSE>(a.e.sc, a.e.q.Lmax, pw);

    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int NW = blockDim.x >> 6;
    const int G = gridDim.x;

    EncStats st;

    DecUnit<SUBD, VW> cur, nxt;
    dec_load<SUBD, VW>(cur, a.d, blockIdx.x, tx, ty, NW);
    for (int t = blockIdx.x; t < a.d.g.totalTiles; t += G) {
        if (a.e.stats) {
            const int f = t / a.d.g.tilesPerFrame;  // wave-uniform
            if (f != st.frame) {
                stats_flush(st, a.e.stats, tx);
                st.frame = f;
            }
        }
        if (cur.valid) {
            EncUnit<VW> u;
            if constexpr (Front::YD) {
                // two copies of the decode arithmetic, chosen by a kernel argument, as in k_decode
                if (kd.sc_mode == 1)
                    dec_values<CSD, SUBD, VW, false, true, true>(cur, a.d, kd, s_lut, s_uv, u.in);
                else
                    dec_values<CSD, SUBD, VW, false, true, false>(cur, a.d, kd, s_lut, s_uv, u.in);
            } else {
                dec_values<CSD, SUBD, VW, true>(cur, a.d, kd, s_lut, s_uv, u.in);
            }
            float c0[2 * VW], c1[2 * VW], c2[2 * VW];
            enc_transform<CSE, VW, Front::YE, false, !Front::YE>(u, a.e, ke, c0, c1, c2, st);
            if constexpr (Front::YE) {
                // channel 0 is t = 219 y + 16 (ycbcr_fwd<., YCODE>); the statistics are about the luminance PQdec(t / 255), which
                // only a launch that asks for them evaluates -- with the complete functions, whose bits the encode kernels' are
                if (a.e.stats) {
#pragma unroll
                    for (int j = 0; j < 2 * VW; j++) {
                        const float lum = pq_decode(div_ieee(c0[j], 255.0f), ke);
                        st.sum += lum;
                        st.mn = fminf(st.mn, lum);
                        st.mx = fmaxf(st.mx, lum);
                    }
                }
            }
            // (the tile, and with it the frame, is wave-uniform: saying so keeps the planes' frame offsets scalar)
            enc_emit<CSE, SUBE, VW, LM>(__builtin_amdgcn_readfirstlane(cur.f), cur.ux, cur.uy, c0, c1, c2, a.e, static_cast<const float *>(nullptr), s_rec);   // (record searches: no table pointer)
        }
        dec_load<SUBD, VW>(nxt, a.d, t + G, tx, ty, NW);
        cur = nxt;
    }
    if (a.e.stats)
        stats_flush(st, a.e.stats, tx);
}

// ---- HALF-RESOLUTION TRANSCODE ----------------------------------------------------------------------
// k_transcode with a 2x2 box in linear light between DEC and ENC: the target planes hold (w/2) x (h/2) luma samples, target pixel
// (X, Y) is m = ((d[2Y][2X] + d[2Y][2X+1]) + (d[2Y+1][2X] + d[2Y+1][2X+1])) * 0.25f of the floats d the decode stores (`/ sc`
// carried out) -- fp32, this association, nothing contracted -- and the planes are what the encode writes for m.  a.d.g is the
// source's geometry (w x h), a.e.g the target's (w/2 x h/2); the loop runs over the target's tiles.  A thread owns the target unit
// (ux, uy), VW pixels x 2 rows, and fills it from the four source units (2ux + i, 2uy + j): source unit (i, j) is VW pixels x 2 rows
// of the source and gives the VW/2 pixels from i * VW/2 on of target row j.  Per lane and row the source reads are two adjacent
// VW-sample pieces, so a wave reads contiguous memory.  w and h are multiples of 4 and VW == 4 only when w/2 is one too
// (transcode_plan), so the source has exactly twice the target's units both ways: the four are in range whenever the target unit is.

// the target unit of tile t for this thread; false: none (the tile overhangs the frame, or t is past the last tile)
LH_DEV bool half_locate(const FrameGeom &g, int t, int tx, int ty, int NW, int &f, int &ux, int &uy)
{
    if (t >= g.totalTiles)
        return false;
    int bx, by;
    tile_coords(t, g, f, bx, by);
    ux = bx * 64 + tx;
    uy = by * NW + ty;
    return ux < g.unitsX && uy < g.unitsY;
}

// How many of a target unit's four source units are loaded one iteration ahead, behind the previous unit's stores (the others are
// loaded where they are decoded).  From the register report (profiles/transcode_half_codegen.txt): a 4:2:0 source unit is VW * 3
// registers, a 4:4:4 one VW * 6.
template <bool SUBD, int VW>
constexpr int half_prefetch()
{
    return VW == 2 ? 4 : 2;
}

// Budget, one function of (CSD, CSE, VW) which the kernel's __launch_bounds__ / amdgpu_waves_per_eu are written with and
// transcode_plan clamps the launch to (profiles/transcode_half_codegen.txt): with YCbCr on either side 512 threads, which leave the
// fp64 powf chains 256 registers, as TransDistBound does for the measuring kernels; Lu'v' -> Lu'v' at VW 4 512 threads and three waves
// per SIMD (168 registers: at 128 the target unit beside a decoded unit and the prefetched ones spill); at VW 2 k_transcode's 1024
constexpr int transhalf_threads_bound(int csd, int cse, int vw)
{
    return (csd == CS_YCBCR || cse == CS_YCBCR || vw == 4) ? 512 : 1024;
}
constexpr int transhalf_waves(int csd, int cse, int vw)
{
    return (csd == CS_YCBCR || cse == CS_YCBCR) ? 2 : vw == 4 ? 3 : 4;
}

// the loads of the first NPF source units of target unit (f, ux, uy): source unit s is (2ux + (s & 1), 2uy + (s >> 1))
template <bool SUBD, int VW, int NPF>
LH_DEV void half_issue(DecUnit<SUBD, VW> (&pf)[NPF], const DecArgs &a, int f, int ux, int uy)
{
    dec_load_at<SUBD, VW>(pf[0], a, f, 2 * ux, 2 * uy);
    if constexpr (NPF > 1)
        dec_load_at<SUBD, VW>(pf[1], a, f, 2 * ux + 1, 2 * uy);
    if constexpr (NPF > 2)
        dec_load_at<SUBD, VW>(pf[2], a, f, 2 * ux, 2 * uy + 1);
    if constexpr (NPF > 3)
        dec_load_at<SUBD, VW>(pf[3], a, f, 2 * ux + 1, 2 * uy + 1);
}

// source unit S of target unit (f, ux, uy) -- prefetched (S < NPF) or loaded here -- decoded and folded into its VW/2 pixels of u.in
template <int S, int CSD, bool SUBD, int VW, bool UVTAB, bool YT, bool SCFAST, int NPF, typename K>
LH_DEV void half_fold(EncUnit<VW> &u, const DecUnit<SUBD, VW> (&pf)[NPF], const DecArgs &a, const K &kd, const float *s_lut, const float *s_uv, int f,
                      int ux, int uy)
{
    constexpr int i = S & 1, j = S >> 1;
    DecUnit<SUBD, VW> du;
    if constexpr (S < NPF)
        du = pf[S];
    else
        dec_load_at<SUBD, VW>(du, a, f, 2 * ux + i, 2 * uy + j);
    float v[3][2][VW];
    dec_values<CSD, SUBD, VW, UVTAB, YT, SCFAST>(du, a, kd, s_lut, s_uv, v);
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int p = 0; p < VW / 2; p++)
            u.in[c][j][i * (VW / 2) + p] = ((v[c][0][2 * p] + v[c][0][2 * p + 1]) + (v[c][1][2 * p] + v[c][1][2 * p + 1])) * 0.25f;
}

// the four source units of a target unit, one at a time: at most one decoded unit is live beside the target unit
template <int CSD, bool SUBD, int VW, bool UVTAB, bool YT, bool SCFAST, int NPF, typename K>
LH_DEV void half_fill(EncUnit<VW> &u, const DecUnit<SUBD, VW> (&pf)[NPF], const DecArgs &a, const K &kd, const float *s_lut, const float *s_uv, int f,
                      int ux, int uy)
{
    half_fold<0, CSD, SUBD, VW, UVTAB, YT, SCFAST>(u, pf, a, kd, s_lut, s_uv, f, ux, uy);
    half_fold<1, CSD, SUBD, VW, UVTAB, YT, SCFAST>(u, pf, a, kd, s_lut, s_uv, f, ux, uy);
    half_fold<2, CSD, SUBD, VW, UVTAB, YT, SCFAST>(u, pf, a, kd, s_lut, s_uv, f, ux, uy);
    half_fold<3, CSD, SUBD, VW, UVTAB, YT, SCFAST>(u, pf, a, kd, s_lut, s_uv, f, ux, uy);
}

// k_transcode_half: k_transcode's tables, statistics and loop order -- the loads of the next target unit's source units are issued
// after the current unit's stores
template <int CSD, bool SUBD, int CSE, bool SUBE, int VW, int LM>
__global__ __launch_bounds__(transhalf_threads_bound(CSD, CSE, VW)) __attribute__((amdgpu_waves_per_eu(transhalf_waves(CSD, CSE, VW))))
void k_transcode_half(const TransArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    using Front = PlaneFront<CSD, CSE, LM>;
    stage_tables<Front::WHAT_D, Front::WHAT_E>(smem, a.d.q, a.e.q);
    constexpr int off = lds_table_offset<Front::WHAT_D | Front::WHAT_E>();
    const float *s_lut = reinterpret_cast<const float *>(smem + off);
    const float *s_uv = reinterpret_cast<const float *>(smem + off + lds_lut_bytes(a.d.q));   // u'v' table, or y table + chroma terms
    const uint32_t *s_rec = reinterpret_cast<const uint32_t *>(smem + off + lds_quant_bytes<Front::WHAT_D>(a.d.q));
    const PowfTablesWide *pw = reinterpret_cast<const PowfTablesWide *>(smem);
    const XformConst kd = make_xform_const<CSD>(a.d.sc, a.d.q.Lmax, pw);
    const XformConst ke = make_xform_const<CSE>(a.e.sc, a.e.q.Lmax, pw);

    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int NW = blockDim.x >> 6;
    const int G = gridDim.x;
    constexpr int NPF = half_prefetch<SUBD, VW>();

    EncStats st;

    DecUnit<SUBD, VW> pf[NPF];
    int f = 0, ux = 0, uy = 0;
    bool valid = half_locate(a.e.g, blockIdx.x, tx, ty, NW, f, ux, uy);
    if (valid)
        half_issue<SUBD, VW>(pf, a.d, f, ux, uy);
    for (int t = blockIdx.x; t < a.e.g.totalTiles; t += G) {
        if (a.e.stats) {
            const int tf = t / a.e.g.tilesPerFrame;  // wave-uniform
            if (tf != st.frame) {
                stats_flush(st, a.e.stats, tx);
                st.frame = tf;
            }
        }
        if (valid) {
            EncUnit<VW> u;
            if constexpr (Front::YD) {
                // two copies of the decode arithmetic, chosen by a kernel argument, as in k_decode
                if (kd.sc_mode == 1)
                    half_fill<CSD, SUBD, VW, false, true, true>(u, pf, a.d, kd, s_lut, s_uv, f, ux, uy);
                else
                    half_fill<CSD, SUBD, VW, false, true, false>(u, pf, a.d, kd, s_lut, s_uv, f, ux, uy);
            } else {
                half_fill<CSD, SUBD, VW, true, false, false>(u, pf, a.d, kd, s_lut, s_uv, f, ux, uy);
            }
            float c0[2 * VW], c1[2 * VW], c2[2 * VW];
            enc_transform<CSE, VW, Front::YE, false, !Front::YE>(u, a.e, ke, c0, c1, c2, st);
            if constexpr (Front::YE) {
                // the luminance statistics of a YCbCr target, only for a launch that asks for them (k_transcode says why)
                if (a.e.stats) {
#pragma unroll
                    for (int j = 0; j < 2 * VW; j++) {
                        const float lum = pq_decode(div_ieee(c0[j], 255.0f), ke);
                        st.sum += lum;
                        st.mn = fminf(st.mn, lum);
                        st.mx = fmaxf(st.mx, lum);
                    }
                }
            }
            // (the tile, and with it the frame, is wave-uniform: saying so keeps the planes' frame offsets scalar)
            enc_emit<CSE, SUBE, VW, LM>(__builtin_amdgcn_readfirstlane(f), ux, uy, c0, c1, c2, a.e, static_cast<const float *>(nullptr), s_rec);   // (record searches: no table pointer)
        }
        valid = half_locate(a.e.g, t + G, tx, ty, NW, f, ux, uy);
        if (valid)
            half_issue<SUBD, VW>(pf, a.d, f, ux, uy);
    }
    if (a.e.stats)
        stats_flush(st, a.e.stats, tx);
}

// ---- QUARTER-RESOLUTION TRANSCODE -------------------------------------------------------------------
// k_transcode_half's 2x2 box applied twice to floats, nothing quantized between the two: the target planes hold (w/4) x (h/4) luma
// samples, target pixel (X, Y) is M = ((m[2Y][2X] + m[2Y][2X+1]) + (m[2Y+1][2X] + m[2Y+1][2X+1])) * 0.25f of the half-size means m
// k_transcode_half encodes -- fp32, this association, nothing contracted -- and the planes are what the encode writes for M.  a.d.g is
// the source's geometry (w x h), a.e.g the target's (w/4 x h/4); the loop runs over the target's tiles (half_locate).  A thread owns
// the target unit (ux, uy), VW pixels x 2 rows, and fills it from the sixteen source units (4ux + i, 4uy + j), i, j in 0..3: source
// unit (i, j) gives the VW/2 means from i * VW/2 on of m's row 4uy + j, which belongs to target row j >> 1 as its upper (j even) or
// lower (j odd) row of means.  Per lane and row the source reads are four adjacent VW-sample pieces whatever the order of the walk, so
// a wave reads contiguous memory.  w and h are multiples of 8 and VW == 4 only when w/4 is a multiple of 4 (transcode_plan), so the
// source has exactly four times the target's units both ways: the sixteen are in range whenever the target unit is.
//
// The walk is a loop that is NOT unrolled, over the 2 * VW target pixels of the unit: step k fills pixel k % VW of row k / VW from
// the source units under it -- VW 4: two, each one's two means a pair-sum, (m00 + m01) from the upper and (m10 + m11) from the lower;
// VW 2: four, one mean each, upper left, upper right, lower left, lower right -- which are decoded one at a time and folded in the
// spec's association; M goes into its place in u.in by selects (the step is wave-uniform, the unit stays in registers).  Unrolled,
// the sixteen copies of the decode arithmetic (twice that for a YCbCr source) made a unit of 5.3 M listing lines whose kernels
// sat at the register cap of every budget (profiles/transcode_quarter_codegen.txt); the loop's body is k_transcode_half's size.  Slot e of step k is source unit (quarter_i, quarter_j).
template <int VW>
constexpr int quarter_slots()
{
    return VW == 4 ? 2 : 4;
}
template <int VW>
LH_DEV int quarter_i(int k, int e)
{
    return VW == 4 ? k % VW : 2 * (k % VW) + (e & 1);
}
template <int VW>
LH_DEV int quarter_j(int k, int e)
{
    return 2 * (k / VW) + (VW == 4 ? e : e >> 1);
}

// How many of a step's slots are loaded ahead (the others are loaded where they are decoded): a slot loaded ahead is refilled with
// the next step's unit right behind its own decode, so that the load runs under the decodes that follow, and after the last step
// with the first step's unit of the thread's next target unit, behind this one's stores.  From the register report
// (profiles/transcode_quarter_codegen.txt): a 4:2:0 source unit is VW * 3 registers, a 4:4:4 one VW * 6, and all of a step's slots
// fit beside the target unit (6 * VW floats) and one decoded unit -- except a 4:4:4 source at VW 2, whose four units ahead (48
// registers) left the four Lu'v' -> Lu'v' kernels 32 B of scratch under their 128 registers: those sources load the upper two ahead.
template <bool SUBD, int VW>
constexpr int quarter_prefetch()
{
    return (VW == 2 && !SUBD) ? 2 : quarter_slots<VW>();
}

// Budget, one function pair of (CSD, CSE, VW) which the kernel's __launch_bounds__ / amdgpu_waves_per_eu are written with and
// transcode_plan clamps the launch to: transhalf_*'s values, which the resource report (profiles/transcode_quarter_codegen.txt) gives
// no reason to move -- the live set is k_transcode_half's plus the step and the sums of the pixel in progress.  With YCbCr on either
// side 512 threads and two waves per SIMD (256 registers for the fp64 powf chains); Lu'v' -> Lu'v' at VW 4 512 threads and three waves
// (168 registers); at VW 2 k_transcode's 1024 threads and four waves (128).
constexpr int transquarter_threads_bound(int csd, int cse, int vw) { return transhalf_threads_bound(csd, cse, vw); }
constexpr int transquarter_waves(int csd, int cse, int vw) { return transhalf_waves(csd, cse, vw); }

// the loads of the slots of step k of target unit (f, ux, uy) that are loaded ahead
template <bool SUBD, int VW, int NPF>
LH_DEV void quarter_issue(DecUnit<SUBD, VW> (&pf)[NPF], const DecArgs &a, int f, int ux, int uy, int k = 0)
{
#pragma unroll
    for (int e = 0; e < NPF; e++)
        dec_load_at<SUBD, VW>(pf[e], a, f, 4 * ux + quarter_i<VW>(k, e), 4 * uy + quarter_j<VW>(k, e));
}

// slot E of step k of target unit (f, ux, uy) -- loaded ahead (E < NPF; then refilled for step k + 1) or loaded here -- decoded: its
// VW/2 half-size means per channel, k_transcode_half's
template <int E, int CSD, bool SUBD, int VW, bool UVTAB, bool YT, bool SCFAST, int NPF, typename K>
LH_DEV void quarter_means(float (&m)[3][VW / 2], DecUnit<SUBD, VW> (&pf)[NPF], const DecArgs &a, const K &kd, const float *s_lut, const float *s_uv, int f,
                          int ux, int uy, int k)
{
    DecUnit<SUBD, VW> du;
    if constexpr (E < NPF)
        du = pf[E];
    else
        dec_load_at<SUBD, VW>(du, a, f, 4 * ux + quarter_i<VW>(k, E), 4 * uy + quarter_j<VW>(k, E));
    float v[3][2][VW];
    dec_values<CSD, SUBD, VW, UVTAB, YT, SCFAST>(du, a, kd, s_lut, s_uv, v);
    if constexpr (E < NPF)
        if (k + 1 < 2 * VW)   // (wave-uniform)
            dec_load_at<SUBD, VW>(pf[E], a, f, 4 * ux + quarter_i<VW>(k + 1, E), 4 * uy + quarter_j<VW>(k + 1, E));
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int p = 0; p < VW / 2; p++)
            m[c][p] = ((v[c][0][2 * p] + v[c][0][2 * p + 1]) + (v[c][1][2 * p] + v[c][1][2 * p + 1])) * 0.25f;
}

// the sixteen source units of a target unit, step by step: at most one decoded unit is live beside the target unit
template <int CSD, bool SUBD, int VW, bool UVTAB, bool YT, bool SCFAST, int NPF, typename K>
LH_DEV void quarter_fill(EncUnit<VW> &u, DecUnit<SUBD, VW> (&pf)[NPF], const DecArgs &a, const K &kd, const float *s_lut, const float *s_uv, int f, int ux,
                         int uy)
{
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int q = 0; q < 2 * VW; q++)
            u.in[c][q / VW][q % VW] = 0.0f;
#pragma unroll 1
    for (int k = 0; k < 2 * VW; k++) {
        float M[3];
        if constexpr (VW == 4) {
            float up[3][2], lo[3][2];
            quarter_means<0, CSD, SUBD, VW, UVTAB, YT, SCFAST>(up, pf, a, kd, s_lut, s_uv, f, ux, uy, k);
            float ps[3];   // the upper pair-sums wait for the lower ones
#pragma unroll
            for (int c = 0; c < 3; c++)
                ps[c] = up[c][0] + up[c][1];
            quarter_means<1, CSD, SUBD, VW, UVTAB, YT, SCFAST>(lo, pf, a, kd, s_lut, s_uv, f, ux, uy, k);
#pragma unroll
            for (int c = 0; c < 3; c++)
                M[c] = (ps[c] + (lo[c][0] + lo[c][1])) * 0.25f;
        } else {
            float m0[3][1], m1[3][1];
            quarter_means<0, CSD, SUBD, VW, UVTAB, YT, SCFAST>(m0, pf, a, kd, s_lut, s_uv, f, ux, uy, k);
            quarter_means<1, CSD, SUBD, VW, UVTAB, YT, SCFAST>(m1, pf, a, kd, s_lut, s_uv, f, ux, uy, k);
            float ps[3];
#pragma unroll
            for (int c = 0; c < 3; c++)
                ps[c] = m0[c][0] + m1[c][0];
            quarter_means<2, CSD, SUBD, VW, UVTAB, YT, SCFAST>(m0, pf, a, kd, s_lut, s_uv, f, ux, uy, k);
            quarter_means<3, CSD, SUBD, VW, UVTAB, YT, SCFAST>(m1, pf, a, kd, s_lut, s_uv, f, ux, uy, k);
#pragma unroll
            for (int c = 0; c < 3; c++)
                M[c] = (ps[c] + (m0[c][0] + m1[c][0])) * 0.25f;
        }
#pragma unroll
        for (int c = 0; c < 3; c++)
#pragma unroll
            for (int q = 0; q < 2 * VW; q++)
                u.in[c][q / VW][q % VW] = q == k ? M[c] : u.in[c][q / VW][q % VW];
    }
}

// k_transcode_quarter: k_transcode_half's tables, statistics and loop order -- the loads of the first steps of the next target unit's
// walk are issued after the current unit's stores
template <int CSD, bool SUBD, int CSE, bool SUBE, int VW, int LM>
__global__ __launch_bounds__(transquarter_threads_bound(CSD, CSE, VW)) __attribute__((amdgpu_waves_per_eu(transquarter_waves(CSD, CSE, VW))))
void k_transcode_quarter(const TransArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    using Front = PlaneFront<CSD, CSE, LM>;
    stage_tables<Front::WHAT_D, Front::WHAT_E>(smem, a.d.q, a.e.q);
    constexpr int off = lds_table_offset<Front::WHAT_D | Front::WHAT_E>();
    const float *s_lut = reinterpret_cast<const float *>(smem + off);
    const float *s_uv = reinterpret_cast<const float *>(smem + off + lds_lut_bytes(a.d.q));   // u'v' table, or y table + chroma terms
    const uint32_t *s_rec = reinterpret_cast<const uint32_t *>(smem + off + lds_quant_bytes<Front::WHAT_D>(a.d.q));
    const PowfTablesWide *pw = reinterpret_cast<const PowfTablesWide *>(smem);
    const XformConst kd = make_xform_const<CSD>(a.d.sc, a.d.q.Lmax, pw);
    const XformConst ke = make_xform_const<CSE>(a.e.sc, a.e.q.Lmax, pw);

    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int NW = blockDim.x >> 6;
    const int G = gridDim.x;
    constexpr int NPF = quarter_prefetch<SUBD, VW>();

    EncStats st;

    DecUnit<SUBD, VW> pf[NPF];
    int f = 0, ux = 0, uy = 0;
    bool valid = half_locate(a.e.g, blockIdx.x, tx, ty, NW, f, ux, uy);
    if (valid)
        quarter_issue<SUBD, VW>(pf, a.d, f, ux, uy);
    for (int t = blockIdx.x; t < a.e.g.totalTiles; t += G) {
        if (a.e.stats) {
            const int tf = t / a.e.g.tilesPerFrame;  // wave-uniform
            if (tf != st.frame) {
                stats_flush(st, a.e.stats, tx);
                st.frame = tf;
            }
        }
        if (valid) {
            EncUnit<VW> u;
            if constexpr (Front::YD) {
                // two copies of the decode arithmetic, chosen by a kernel argument, as in k_decode
                if (kd.sc_mode == 1)
                    quarter_fill<CSD, SUBD, VW, false, true, true>(u, pf, a.d, kd, s_lut, s_uv, f, ux, uy);
                else
                    quarter_fill<CSD, SUBD, VW, false, true, false>(u, pf, a.d, kd, s_lut, s_uv, f, ux, uy);
            } else {
                quarter_fill<CSD, SUBD, VW, true, false, false>(u, pf, a.d, kd, s_lut, s_uv, f, ux, uy);
            }
            float c0[2 * VW], c1[2 * VW], c2[2 * VW];
            enc_transform<CSE, VW, Front::YE, false, !Front::YE>(u, a.e, ke, c0, c1, c2, st);
            if constexpr (Front::YE) {
                // the luminance statistics of a YCbCr target, only for a launch that asks for them (k_transcode says why)
                if (a.e.stats) {
#pragma unroll
                    for (int j = 0; j < 2 * VW; j++) {
                        const float lum = pq_decode(div_ieee(c0[j], 255.0f), ke);
                        st.sum += lum;
                        st.mn = fminf(st.mn, lum);
                        st.mx = fmaxf(st.mx, lum);
                    }
                }
            }
            // (the tile, and with it the frame, is wave-uniform: saying so keeps the planes' frame offsets scalar)
            enc_emit<CSE, SUBE, VW, LM>(__builtin_amdgcn_readfirstlane(f), ux, uy, c0, c1, c2, a.e, static_cast<const float *>(nullptr), s_rec);   // (record searches: no table pointer)
        }
        valid = half_locate(a.e.g, t + G, tx, ty, NW, f, ux, uy);
        if (valid)
            quarter_issue<SUBD, VW>(pf, a.d, f, ux, uy);
    }
    if (a.e.stats)
        stats_flush(st, a.e.stats, tx);
}

// The decoded-and-transformed channel 0 of one frame, pixel by pixel with the complete functions (the array the reference's
// sequential mean sums, k_seq_sum): only for the host call's rare exact mean (lumahip_transcode_frame_host).
struct TransChan0Args {
    QuantDev qd;
    const unsigned char *src[3];
    int stride[3];
    int bps, sub, w, h;
    float sc_src, sc_dst, Lmax_dst;
    float *out;
};

template <int CSD, int CSE>
__global__ __launch_bounds__(256) void k_transcode_channel0(const TransChan0Args a)
{
    __shared__ __attribute__((aligned(16))) unsigned char s_raw[(CSD == CS_YCBCR || CSE == CS_YCBCR) ? sizeof(PowfTablesWide) : 16];
    PowfTablesWide &s_pw = *reinterpret_cast<PowfTablesWide *>(s_raw);
    if constexpr (CSD == CS_YCBCR || CSE == CS_YCBCR) {
        stage_powf_tables(&s_pw);
        __syncthreads();
    }
    const XformConst kd = make_xform_const<CSD>(a.sc_src, a.qd.Lmax, &s_pw), ke = make_xform_const<CSE>(a.sc_dst, a.Lmax_dst, &s_pw);
    const size_t n = (size_t)a.w * a.h;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int y = (int)(i / a.w), x = (int)(i - (size_t)y * a.w);
        const int yc = a.sub ? y / 2 : y, xc = a.sub ? x / 2 : x;
        int s0[1], s1[1], s2[1];
        load_samples<1>(a.src[0] + (size_t)y * a.stride[0] + (size_t)x * a.bps, s0, a.bps, 0);
        load_samples<1>(a.src[1] + (size_t)yc * a.stride[1] + (size_t)xc * a.bps, s1, a.bps, 0);
        load_samples<1>(a.src[2] + (size_t)yc * a.stride[2] + (size_t)xc * a.bps, s2, a.bps, 0);
        float r, g, b, c0, c1, c2;
        xform_inv<CSD>(dequantize_lut(s0[0], a.qd.lut, a.qd.maxVal), dequantize_color(s1[0], a.qd.maxC), dequantize_color(s2[0], a.qd.maxC), kd, r, g, b);
        r = div_ieee(r, a.sc_src);
        g = div_ieee(g, a.sc_src);
        b = div_ieee(b, a.sc_src);
        xform_fwd<CSE>(r * a.sc_dst, g * a.sc_dst, b * a.sc_dst, ke, c0, c1, c2);
        a.out[i] = c0;
    }
}

// ---- DISTORTION -------------------------------------------------------------------------------------
// How far GIVEN code planes are from the planes k_encode would write for the same frames: per frame and plane the integer sums
// {sum (e-g)^2, sum |e-g|, max |e-g|, #(e != g)} over the plane's samples, e = the sample k_encode stores (masked to the profile's
// sample width exactly as store_samples packs it), g = the sample that is there, as the decoder reads it.  Reads 12 + 3 B per pixel
// (6 + 3 from binary16 frames), writes 12 words per frame.
// The given samples are the decode kernels' own prefetch (dec_issue: load_samples' vector loads without the unpack; rows they
// cannot take go through load_samples itself, later): issued right behind the next unit's pixel loads, one iteration ahead, and
// unpacked row by row where the codes are compared -- the wait for the pixels (loads complete in order) leaves them in flight.
// Accumulation: 64 bits per lane for the two sums (one squared difference of 16-bit samples fills 32); one 64-bit integer atomic
// per workgroup, frame and word reaches out[] (thousands of waves on one address is what profiles/r03_hostfed_trace.txt records).
// Integers throughout: the result does not depend on the launch shape or on the order of arrival.
struct DistArgs {
    EncArgs e;       // q (the composite records for LM 5 / 6), g, src, frame_stride, sc, half of the frames; dst / stride / bps unused
    DecArgs g;       // the given planes: src, stride, src_frame_stride, bps, aligned; g (the same geometry as e.g)
    uint64_t *out;   // [nframes][3 planes][sse, sad, max_abs, n_differ], zeroed before the launch
};

struct DistAcc {
    uint64_t sse[3], sad[3];
    uint32_t mx[3], nd[3];   // (a lane's share of one frame is far below 2^32 samples)
    int frame = -1;          // no frame yet
    LH_DEVS DistAcc() { reset(); }
    LH_DEVS void reset()
    {
#pragma unroll
        for (int p = 0; p < 3; p++) {
            sse[p] = sad[p] = 0;
            mx[p] = nd[p] = 0;
        }
    }
};

// the consumer of enc_codes that measures: each row handed over against the same row of the given unit, unpacked from the
// prefetched words `g` only now (rows the vector loads could not take are loaded here, byte by byte, as dec_finish does)
// Acc: where the lane's sums go -- DistAcc (a frame's) or DistBlockAcc (a map block's, k_distortion_map)
template <bool SUB, int VW, typename Acc = DistAcc>
struct DistMeasureUnit {
    const DecRaw<SUB, VW> &g;
    const DecArgs &d;
    Acc &acc;
    int mask;   // 0xffff / 0xff: what store_samples keeps of a code
    template <int N>
    LH_DEVS void row(int pl, int r, const int (&codes)[N]) const
    {
        int given[N];
        if (d.aligned) {   // (given_row's lines, written out: see there)
            unpack_raw<N>(pl == 0 ? g.y[r] : pl == 1 ? g.c1[r] : g.c2[r], given, d.bps);
        } else {
            load_samples<N>(dec_row<SUB>(d, pl, g.f, g.ux, g.uy, r, N), given, d.bps, 0);
        }
#pragma unroll
        for (int i = 0; i < N; i++) {
            const int df = (codes[i] & mask) - given[i];
            const uint32_t ad = (uint32_t)(df < 0 ? -df : df);   // <= 65535: ad * ad fits 32 bits
            acc.sse[pl] += (uint64_t)(ad * ad);
            acc.sad[pl] += ad;
            acc.mx[pl] = ad > acc.mx[pl] ? ad : acc.mx[pl];
            acc.nd[pl] += ad != 0;
        }
    }
};

// The 12 words of LDS in which the lanes of a measuring workgroup that saw a difference meet (LDS atomics), zeroed: called before
// the front end's stage_tables, which synchronises.  Must stay LH_DEV: force-inlined, the array is the calling kernel's
LH_DEV unsigned long long *dist_words()
{
    __shared__ unsigned long long s_acc[12];
    if (threadIdx.x < 12)
        s_acc[threadIdx.x] = 0;
    return s_acc;
}

// The one flush site, at the top of every iteration of a measuring loop: f = the frame of the iteration's tile, or -2 past the last
// tile (the loop then leaves).  Every thread of the workgroup calls it at the same point (the frame index is workgroup-uniform).
// When the frame changes the lanes meet in s_acc, then one thread per word hands it to out[frame * 12 + .] and clears it -- a flush
// happens once per workgroup and frame, not per unit
LH_DEV void dist_flush(DistAcc &acc, unsigned long long *s_acc, int f, uint64_t *out)
{
    if (f != acc.frame) {
        if (acc.frame >= 0) {
#pragma unroll
            for (int p = 0; p < 3; p++)
                if (acc.nd[p] != 0) {
                    atomicAdd(&s_acc[4 * p + 0], (unsigned long long)acc.sse[p]);
                    atomicAdd(&s_acc[4 * p + 1], (unsigned long long)acc.sad[p]);
                    atomicMax(&s_acc[4 * p + 2], (unsigned long long)acc.mx[p]);
                    atomicAdd(&s_acc[4 * p + 3], (unsigned long long)acc.nd[p]);
                }
            __syncthreads();
            if (threadIdx.x < 12) {
                const unsigned long long v = s_acc[threadIdx.x];
                s_acc[threadIdx.x] = 0;
                unsigned long long *dst = reinterpret_cast<unsigned long long *>(out) + (size_t)acc.frame * 12 + threadIdx.x;
                if (v != 0) {
                    if ((threadIdx.x & 3) == 2)
                        atomicMax(dst, v);
                    else
                        atomicAdd(dst, v);
                }
            }
            __syncthreads();
        }
        acc.reset();
        acc.frame = f;
    }
}

// k_distortion: LM 3 / 7 (the luminance records in LDS), 5 (YCbCr: the composite records), 6 (5 + the half-input table; binary16
// frames).  k_encode's loop; the given words of a unit travel with its pixels.
// Register budget: four waves per SIMD for every variant -- the accumulators (18 registers) and the given words in flight (up to
// 8) do not fit the 80 registers of the light k_encode variants, and the launch rules run three 256-thread workgroups per CU anyway.
template <int CS, bool SUB, int VW, int LM, bool IN16 = false>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(4))) void k_distortion(const DistArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    static_assert(LM == 3 || LM == 7 || LM == 5 || LM == 6, "search records in LDS");
    unsigned long long *const s_acc = dist_words();
    stage_tables<FrameFront<CS, LM>::WHAT>(smem, a.e.q, a.e.half);
    const FrameFront<CS, LM> fr(smem, a.e);

    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int NW = blockDim.x >> 6;
    const int G = gridDim.x;

    const int mask = a.g.bps == 2 ? 0xffff : 0xff;
    DistAcc acc;
    EncStats st;   // (enc_transform's parameter; unused with STATS = false)
    EncUnit<VW> u;
    DecRaw<SUB, VW> given;
    enc_load<VW, IN16>(u, a.e, blockIdx.x, tx, ty, NW);
    dec_issue<SUB, VW>(given, a.g, blockIdx.x, tx, ty, NW);
    for (int t = blockIdx.x;; t += G) {
        const bool done = t >= a.e.g.totalTiles;        // workgroup-uniform, as the frame index is
        dist_flush(acc, s_acc, done ? -2 : t / a.e.g.tilesPerFrame, a.out);
        if (done)
            break;
        if (u.valid) {
            float c0[2 * VW], c1[2 * VW], c2[2 * VW];
            enc_transform<CS, VW, LM == 5 || LM == 6, LM == 6, false>(u, a.e, fr.k, c0, c1, c2, st, fr.s_half);
            const DistMeasureUnit<SUB, VW> out{given, a.g, acc, mask};
            enc_codes<CS, SUB, VW, LM == 6 ? 5 : LM>(c0, c1, c2, a.e.q, static_cast<const float *>(nullptr), fr.s_rec, out);   // (record searches: no table pointer)
        }
        enc_load<VW, IN16>(u, a.e, t + G, tx, ty, NW);
        dec_issue<SUB, VW>(given, a.g, t + G, tx, ty, NW);
    }
}

// ---- TRANSCODE DISTORTION ---------------------------------------------------------------------------
// How far GIVEN code planes are from the planes k_transcode would write for the same source planes.  Reads 3 + 3 B per pixel
// (profile 2 on both sides), writes 12 words per frame; no scratch planes, no float frame.  The given samples travel as
// k_distortion's do, under the TARGET's subsampling and sample size, their loads right behind the next unit's source loads.
struct TransDistArgs {
    DecArgs d;       // the source planes, as TransArgs::d
    EncArgs e;       // the target quantizer: q (the composite records for LM == 5), g, sc; nothing is stored
    DecArgs g;       // the given planes: src, stride, src_frame_stride, bps, aligned; g (the same geometry as d.g)
    uint64_t *out;   // [nframes][3 planes][sse, sad, max_abs, n_differ], zeroed before the launch
};

// Threads per workgroup the variants are register-allocated for: the pairs with YCbCr on either side already sit at 111 - 128
// registers in k_transcode and the measuring consumer adds the accumulators (18) and the given words (up to 8), which does not fit
// the 64 registers of a 1024-thread workgroup without scratch -- they are bounded at 512 threads (128 registers), which is what the
// launch rules give them anyway (block_threads_for, valu_bound), and the dispatcher clamps forced or table-driven larger
// workgroups to it.  The Lu'v' -> Lu'v' pairs keep 1024: their tables alone decide the workgroup size.
template <int CSD, int CSE>
struct TransDistBound {
    static constexpr int value = (CSD == CS_YCBCR || CSE == CS_YCBCR) ? 512 : 1024;
};

// k_transcode's loop with the given words travelling beside the source codes
template <int CSD, bool SUBD, int CSE, bool SUBE, int VW, int LM>
__global__ __launch_bounds__((TransDistBound<CSD, CSE>::value)) void k_transcode_distortion(const TransDistArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned long long *const s_acc = dist_words();
    using Front = PlaneFront<CSD, CSE, LM>;
    stage_tables<Front::WHAT_D, Front::WHAT_E>(smem, a.d.q, a.e.q);
    constexpr int off = lds_table_offset<Front::WHAT_D | Front::WHAT_E>();
    const float *s_lut = reinterpret_cast<const float *>(smem + off);
    const float *s_uv = reinterpret_cast<const float *>(smem + off + lds_lut_bytes(a.d.q));   // u'v' table, or y table + chroma terms
    const uint32_t *s_rec = reinterpret_cast<const uint32_t *>(smem + off + lds_quant_bytes<Front::WHAT_D>(a.d.q));
    const PowfTablesWide *pw = reinterpret_cast<const PowfTablesWide *>(smem);
    const XformConst kd = make_xform_const<CSD>(a.d.sc, a.d.q.Lmax, pw);
    const XformConst ke = make_xform_const<CSE>(a.e.sc, a.e.q.Lmax, pw);

    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int NW = blockDim.x >> 6;
    const int G = gridDim.x;

    const int mask = a.g.bps == 2 ? 0xffff : 0xff;
    DistAcc acc;
    EncStats st;   // (enc_transform's parameter; unused with STATS = false)
    DecUnit<SUBD, VW> cur, nxt;
    DecRaw<SUBE, VW> given;
    dec_load<SUBD, VW>(cur, a.d, blockIdx.x, tx, ty, NW);
    dec_issue<SUBE, VW>(given, a.g, blockIdx.x, tx, ty, NW);
    for (int t = blockIdx.x;; t += G) {
        const bool done = t >= a.d.g.totalTiles;
        dist_flush(acc, s_acc, done ? -2 : t / a.d.g.tilesPerFrame, a.out);
        if (done)
            break;
        if (cur.valid) {
            EncUnit<VW> u;
            if constexpr (Front::YD) {
                // two copies of the decode arithmetic, chosen by a kernel argument, as in k_decode
                if (kd.sc_mode == 1)
                    dec_values<CSD, SUBD, VW, false, true, true>(cur, a.d, kd, s_lut, s_uv, u.in);
                else
                    dec_values<CSD, SUBD, VW, false, true, false>(cur, a.d, kd, s_lut, s_uv, u.in);
            } else {
                dec_values<CSD, SUBD, VW, true>(cur, a.d, kd, s_lut, s_uv, u.in);
            }
            float c0[2 * VW], c1[2 * VW], c2[2 * VW];
            enc_transform<CSE, VW, Front::YE, false, false>(u, a.e, ke, c0, c1, c2, st);
            const DistMeasureUnit<SUBE, VW> out{given, a.g, acc, mask};
            enc_codes<CSE, SUBE, VW, LM>(c0, c1, c2, a.e.q, static_cast<const float *>(nullptr), s_rec, out);   // (record searches: no table pointer)
        }
        dec_load<SUBD, VW>(nxt, a.d, t + G, tx, ty, NW);
        dec_issue<SUBE, VW>(given, a.g, t + G, tx, ty, NW);
        cur = nxt;
    }
}

// ---- DISTORTION MAP ---------------------------------------------------------------------------------
// k_distortion's four words per plane for every B x B block of luma pixels (B = 16, 32 or 64; a 4:2:0 chroma plane: the samples
// co-sited with them): map[(((f * nby + by) * nbx + bx) * 3 + p) * 4 + k].  Front end, given-plane prefetch and comparison are
// k_distortion's; what differs is the accumulation in space, and it has an owner for every word: a workgroup owns whole blocks and
// writes their words with plain stores -- no global atomic, no memset in front of the launch, every word written exactly once.
//   - A MAP TILE is S = B / (2 NW) vertically consecutive standard tiles (64 VW pixels x 2 NW rows) of one frame: 64 VW / B blocks
//     side by side, whole.  The workgroup walks its sub-tiles with enc_load / dec_issue (map_subtile names them; one past the last
//     tile row of a frame is never formed), the lanes keep their sums across the S steps (DistBlockAcc).
//   - At the end of a map tile the B / VW adjacent lanes that hold a block's columns add up among themselves (map_lanes_meet: DPP
//     within a row of 16 lanes, one swizzle for 32), the first lane of each group adds into the block's 12 words of LDS, where the
//     NW waves meet, and after a barrier the workgroup stores the tile's blocks that lie inside the map -- contiguous words -- and
//     clears them for the next map tile.
// Integers throughout: the map does not depend on the launch shape.
// What the map's helpers read beside the launch's frame-major FrameGeom, which they take from either front end's arguments (the
// frame-fed kernel's is EncArgs::g, the plane-fed one's DecArgs::g)
struct MapGeom {
    int B, S;          // block size in luma pixels; sub-tiles per map tile, B / (2 NW) >= 1 (the host clamps the workgroup)
    int nbx, nby;      // blocks per frame: ceil(w / B), ceil(h / B)
    int mapTilesPerFrame, totalMapTiles;   // nby * g.tilesX, * nframes
};

// (of both frame-fed map kernels, k_distortion_map and k_moments_map)
struct MapArgs {
    EncArgs e;         // as DistArgs::e
    DecArgs g;         // as DistArgs::g
    uint64_t *map;     // [nframes][nby][nbx][3 planes][sse, sad, max_abs, n_differ | se, sg, see, sgg, seg]; needs no zeroing
    MapGeom m;
};

// What a map kernel's helpers (dist_map_words, map_lanes_meet, dist_map_flush) ask of a lane's per-block record: WORDS per block
// in LDS and in the map, MIN_B the smallest block its calls accept (a map tile holds up to 256 / MIN_B blocks: map_lds_words), and
// the overloads map_lanes_step / map_wave_has / map_lanes_add below.
// a lane's share of ONE block: at most 64 rows x 4 columns, so only the squares need 64 bits -- and so do their sums over a block
struct DistBlockAcc {
    static constexpr int WORDS = 12, MIN_B = 16;
    uint64_t sse[3];
    uint32_t sad[3], mx[3], nd[3];
    LH_DEVS DistBlockAcc() { reset(); }
    LH_DEVS void reset()
    {
#pragma unroll
        for (int p = 0; p < 3; p++) {
            sse[p] = 0;
            sad[p] = mx[p] = nd[p] = 0;
        }
    }
};

// The moments of both signals (k_moments_map): sum e, sum g, sum e^2, sum g^2, sum e g of a lane's share of ONE block.  256 samples
// of at most 65535: the first moments fit 32 bits (< 2^24), a product of two samples fills 32 and their sums need 64.
struct MomentBlockAcc {
    static constexpr int WORDS = 15, MIN_B = 8;
    uint32_t se[3], sg[3];
    uint64_t see[3], sgg[3], seg[3];
    LH_DEVS MomentBlockAcc() { reset(); }
    LH_DEVS void reset()
    {
#pragma unroll
        for (int p = 0; p < 3; p++) {
            se[p] = sg[p] = 0;
            see[p] = sgg[p] = seg[p] = 0;
        }
    }
};

// LDS words the blocks of a map tile meet in: 64 VW / B <= 256 / MIN_B blocks per map tile
template <typename Acc>
constexpr int map_lds_words() { return 256 / Acc::MIN_B * Acc::WORDS; }
constexpr int DIST_MAP_LDS_WORDS = map_lds_words<DistBlockAcc>();       // 16 x 12: 1536 B
constexpr int MOMENTS_MAP_LDS_WORDS = map_lds_words<MomentBlockAcc>();  // 32 x 15: 3840 B

// the map's LDS words, zeroed (as dist_words: before stage_tables, which synchronises; force-inlined, the array is the kernel's)
template <typename Acc = DistBlockAcc>
LH_DEV unsigned long long *dist_map_words()
{
    __shared__ unsigned long long s_map[map_lds_words<Acc>()];
    for (int i = threadIdx.x; i < map_lds_words<Acc>(); i += blockDim.x)
        s_map[i] = 0;
    return s_map;
}

// Standard tile of sub-tile s of map tile m in the frame-major geometry, or totalTiles ("no tile" to enc_load / dec_load / dec_issue) past
// the last map tile and past the frame's last tile row (h not a multiple of B: the last block row has fewer sub-tiles).  Scalar.
LH_DEV int map_subtile(const MapGeom &a, const FrameGeom &g, int m, int s)
{
    if (m >= a.totalMapTiles)
        return g.totalTiles;
    const int f = m / a.mapTilesPerFrame, r = m - f * a.mapTilesPerFrame;
    const int by = r / g.tilesX, bx = r - by * g.tilesX;
    const int row = by * a.S + s;
    if (row >= g.tilesY)
        return g.totalTiles;
    return f * g.tilesPerFrame + row * g.tilesX + bx;
}

template <int CTRL>
LH_DEV uint32_t dpp_lane(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, false); }
// v of the lane 16 away within each half of the wave (bit-mask swizzle: and 0x1f, or 0, xor 0x10); moves no LDS data
LH_DEV uint32_t swz16_lane(uint32_t v) { return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x401f); }

// one step of the meeting of a block's lanes: every lane takes in the sums of the lane Xch names
template <typename Xch>
LH_DEV void map_lanes_step(DistBlockAcc &acc, Xch xch)
{
#pragma unroll
    for (int p = 0; p < 3; p++) {
        const uint32_t lo = xch((uint32_t)acc.sse[p]), hi = xch((uint32_t)(acc.sse[p] >> 32));
        acc.sse[p] += ((uint64_t)hi << 32) | lo;
        acc.sad[p] += xch(acc.sad[p]);
        const uint32_t m = xch(acc.mx[p]);
        acc.mx[p] = m > acc.mx[p] ? m : acc.mx[p];
        acc.nd[p] += xch(acc.nd[p]);
    }
}

template <typename Xch>
LH_DEV void map_lanes_step(MomentBlockAcc &acc, Xch xch)
{
    const auto x64 = [&](uint64_t v) { return ((uint64_t)xch((uint32_t)(v >> 32)) << 32) | xch((uint32_t)v); };
#pragma unroll
    for (int p = 0; p < 3; p++) {
        acc.se[p] += xch(acc.se[p]);
        acc.sg[p] += xch(acc.sg[p]);
        acc.see[p] += x64(acc.see[p]);
        acc.sgg[p] += x64(acc.sgg[p]);
        acc.seg[p] += x64(acc.seg[p]);
    }
}

// The `lanes` (2 -- blocks of 8 at VW 4, MomentBlockAcc only --, 4, 8, 16 or 32; uniform) adjacent lanes of a block, aligned to that
// count: afterwards every one of them holds the block's sums over this wave's rows.  Pairs, then quads (quad_perm), the other quad of
// eight (row_half_mirror: its lanes hold the same sums by then), the other eight of a row (row_mirror), the other row of 32
template <typename Acc>
LH_DEV void map_lanes_meet(Acc &acc, int lanes)
{
    map_lanes_step(acc, [](uint32_t v) { return dpp_lane<0xb1>(v); });   // quad_perm [1, 0, 3, 2]
    if (Acc::MIN_B >= 16 || lanes >= 4)   // (a record whose smallest block is 16 never meets in pairs only)
        map_lanes_step(acc, [](uint32_t v) { return dpp_lane<0x4e>(v); });   // quad_perm [2, 3, 0, 1]
    if (lanes >= 8)
        map_lanes_step(acc, [](uint32_t v) { return dpp_lane<0x141>(v); });   // row_half_mirror
    if (lanes >= 16)
        map_lanes_step(acc, [](uint32_t v) { return dpp_lane<0x140>(v); });   // row_mirror
    if (lanes >= 32)
        map_lanes_step(acc, [](uint32_t v) { return swz16_lane(v); });
}

// whether this wave has anything to add to the LDS words (uniform).  Differences: a wave that saw none anywhere has not -- the words
// are zero already.  Moments: always -- they are non-zero for identical planes
LH_DEV bool map_wave_has(const DistBlockAcc &acc) { return __builtin_amdgcn_ballot_w64((acc.nd[0] | acc.nd[1] | acc.nd[2]) != 0) != 0; }
LH_DEV bool map_wave_has(const MomentBlockAcc &) { return true; }

// the first lane of a block's group adds the group's sums into the block's words w
LH_DEV void map_lanes_add(const DistBlockAcc &acc, unsigned long long *w)
{
#pragma unroll
    for (int p = 0; p < 3; p++)
        if (acc.nd[p] != 0) {
            atomicAdd(&w[4 * p + 0], (unsigned long long)acc.sse[p]);
            atomicAdd(&w[4 * p + 1], (unsigned long long)acc.sad[p]);
            atomicMax(&w[4 * p + 2], (unsigned long long)acc.mx[p]);
            atomicAdd(&w[4 * p + 3], (unsigned long long)acc.nd[p]);
        }
}
LH_DEV void map_lanes_add(const MomentBlockAcc &acc, unsigned long long *w)
{
#pragma unroll
    for (int p = 0; p < 3; p++) {
        atomicAdd(&w[5 * p + 0], (unsigned long long)acc.se[p]);
        atomicAdd(&w[5 * p + 1], (unsigned long long)acc.sg[p]);
        atomicAdd(&w[5 * p + 2], (unsigned long long)acc.see[p]);
        atomicAdd(&w[5 * p + 3], (unsigned long long)acc.sgg[p]);
        atomicAdd(&w[5 * p + 4], (unsigned long long)acc.seg[p]);
    }
}

// The end of map tile m, called by every thread of the workgroup at the same point (m is workgroup-uniform): lanes, waves, stores.
template <int VW, typename Acc>
LH_DEV void dist_map_flush(Acc &acc, unsigned long long *s_map, const MapGeom &a, const FrameGeom &g, uint64_t *map, int m, int tx)
{
    constexpr int W = Acc::WORDS;
    const int lanes = a.B / VW;                    // of a wave per block: (2,) 4 ... 32, a power of two
    const int lanes_log2 = __builtin_ctz(lanes);   // (uniform)
    if (map_wave_has(acc)) {
        map_lanes_meet(acc, lanes);
        if ((tx & (lanes - 1)) == 0)   // (every lane adding into LDS itself measured no better: profiles/map_lanes_ab.txt)
            map_lanes_add(acc, s_map + (tx >> lanes_log2) * W);
    }
    __syncthreads();
    const int f = m / a.mapTilesPerFrame, r = m - f * a.mapTilesPerFrame;
    const int by = r / g.tilesX, bx = r - by * g.tilesX;
    const int b0 = bx * (64 >> lanes_log2);          // the tile's first block: inside the map, as the tile is
    const int nb = min(64 >> lanes_log2, a.nbx - b0);   // (blocks past nbx hold no pixel: their words stayed zero)
    unsigned long long *dst = reinterpret_cast<unsigned long long *>(map) + (((size_t)f * a.nby + by) * a.nbx + b0) * W;
    for (int i = threadIdx.x; i < nb * W; i += blockDim.x) {
        dst[i] = s_map[i];
        s_map[i] = 0;
    }
    __syncthreads();
}

// k_distortion's variants and register budget.  The loop is k_distortion's over the sub-tiles of the workgroup's map tiles: the
// loads of the next sub-tile -- of the next map tile behind the last one -- are issued before the flush, so they are in flight
// across its barriers.
template <int CS, bool SUB, int VW, int LM, bool IN16 = false>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(4))) void k_distortion_map(const MapArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    static_assert(LM == 3 || LM == 7 || LM == 5 || LM == 6, "search records in LDS");
    unsigned long long *const s_map = dist_map_words();
    stage_tables<FrameFront<CS, LM>::WHAT>(smem, a.e.q, a.e.half);
    const FrameFront<CS, LM> fr(smem, a.e);

    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int NW = blockDim.x >> 6;
    const int G = gridDim.x;

    const int mask = a.g.bps == 2 ? 0xffff : 0xff;
    DistBlockAcc acc;
    EncStats st;   // (enc_transform's parameter; unused with STATS = false)
    EncUnit<VW> u;
    DecRaw<SUB, VW> given;
    int m = blockIdx.x, s = 0;
    {
        const int t = map_subtile(a.m, a.e.g, m, 0);
        enc_load<VW, IN16>(u, a.e, t, tx, ty, NW);
        dec_issue<SUB, VW>(given, a.g, t, tx, ty, NW);
    }
    while (m < a.m.totalMapTiles) {   // workgroup-uniform
        if (u.valid) {
            float c0[2 * VW], c1[2 * VW], c2[2 * VW];
            enc_transform<CS, VW, LM == 5 || LM == 6, LM == 6, false>(u, a.e, fr.k, c0, c1, c2, st, fr.s_half);
            const DistMeasureUnit<SUB, VW, DistBlockAcc> out{given, a.g, acc, mask};
            enc_codes<CS, SUB, VW, LM == 6 ? 5 : LM>(c0, c1, c2, a.e.q, static_cast<const float *>(nullptr), fr.s_rec, out);   // (record searches: no table pointer)
        }
        const bool last = s + 1 == a.m.S;
        const int mn = last ? m + G : m, sn = last ? 0 : s + 1;
        const int t = map_subtile(a.m, a.e.g, mn, sn);
        enc_load<VW, IN16>(u, a.e, t, tx, ty, NW);
        dec_issue<SUB, VW>(given, a.g, t, tx, ty, NW);
        if (last) {
            dist_map_flush<VW>(acc, s_map, a.m, a.e.g, a.map, m, tx);
            acc.reset();
        }
        m = mn;
        s = sn;
    }
}

// ---- MOMENTS MAP ------------------------------------------------------------------------------------
// What a structural-similarity index in the code domain needs of every B x B block of luma pixels (B = 8, 16, 32 or 64; block
// membership is the distortion map's): per plane the five sums {sum e, sum g, sum e^2, sum g^2, sum e g} over the block's samples, e and
// g exactly k_distortion_map's -- map[(((f * nby + by) * nbx + bx) * 3 + p) * 5 + k].  sum e^2 - 2 sum e g + sum g^2 is that map's sse.
// k_distortion_map's front end, loop, prefetch order, flush site and owner per word with another consumer (MomentMeasureUnit) and
// another record (MomentBlockAcc): 15 words per block, LDS adds only, no shortcut for waves without a difference.  B = 8 makes a
// block 2 lanes at VW 4 (map_lanes_meet's pair step alone) and a map tile 32 blocks.
// Reads 12 + 3 B per pixel (6 + 3 from binary16 frames), writes 120 B per block; no scratch planes, no global atomic, no memset.
// Row r of plane pl of the given unit: the prefetched words where the set is `aligned`, else loaded here.  DistMeasureUnit::row
// keeps these four lines written out (the address itself is dec_row's in both): calling this function from there, tried again with
// dec_row in place, still gives every k_distortion(_map), k_transcode_distortion(_map) and k_planes_distortion(_map) kernel other
// instruction counts or orders (profiles/plane_loads_codegen.txt, and before it profiles/moments_map_codegen.txt).
template <bool SUB, int VW, int N>
LH_DEV void given_row(const DecRaw<SUB, VW> &g, const DecArgs &d, int pl, int r, int (&given)[N])
{
    if (d.aligned) {
        unpack_raw<N>(pl == 0 ? g.y[r] : pl == 1 ? g.c1[r] : g.c2[r], given, d.bps);
    } else {
        load_samples<N>(dec_row<SUB>(d, pl, g.f, g.ux, g.uy, r, N), given, d.bps, 0);
    }
}

// the consumer of enc_codes that accumulates the moments of both signals, row by row
template <bool SUB, int VW>
struct MomentMeasureUnit {
    const DecRaw<SUB, VW> &g;
    const DecArgs &d;
    MomentBlockAcc &acc;
    int mask;   // 0xffff / 0xff: what store_samples keeps of a code
    template <int N>
    LH_DEVS void row(int pl, int r, const int (&codes)[N]) const
    {
        int given[N];
        given_row<SUB, VW, N>(g, d, pl, r, given);
#pragma unroll
        for (int i = 0; i < N; i++) {
            const uint32_t e = (uint32_t)(codes[i] & mask), gv = (uint32_t)given[i];   // <= 65535: a product fits 32 bits
            acc.se[pl] += e;
            acc.sg[pl] += gv;
            acc.see[pl] += (uint64_t)(e * e);
            acc.sgg[pl] += (uint64_t)(gv * gv);
            acc.seg[pl] += (uint64_t)(e * gv);
        }
    }
};

// Register budget (DESIGN.md 3.11 has the compiler's table): the record is 24 registers against DistBlockAcc's 15.  The variants
// that fit 128 registers with it keep k_distortion_map's bound -- 1024 threads, four waves per SIMD; those that would spill there
// (moments_wide) are allocated for three waves per SIMD (168 registers) in workgroups of at most 512 threads, which distortion_plan
// clamps the launch to (moments_threads_bound).
constexpr bool moments_wide(int cs, bool sub, int vw, int lm)
{
    // every VW 2 variant fits 128 registers, and so do the 4:2:0 RGB / XYZ ones at VW 4; whatever the search mode
    (void)lm;
    return vw == 4 && !((cs == CS_RGB || cs == CS_XYZ) && sub);
}
constexpr int moments_threads_bound(int cs, bool sub, int vw, int lm) { return moments_wide(cs, sub, vw, lm) ? 512 : 1024; }

template <int CS, bool SUB, int VW, int LM, bool IN16 = false>
__global__ __launch_bounds__(moments_threads_bound(CS, SUB, VW, LM)) __attribute__((amdgpu_waves_per_eu(moments_wide(CS, SUB, VW, LM) ? 3 : 4)))
void k_moments_map(const MapArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    static_assert(LM == 3 || LM == 7 || LM == 5 || LM == 6, "search records in LDS");
    unsigned long long *const s_map = dist_map_words<MomentBlockAcc>();
    stage_tables<FrameFront<CS, LM>::WHAT>(smem, a.e.q, a.e.half);
    const FrameFront<CS, LM> fr(smem, a.e);

    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int NW = blockDim.x >> 6;
    const int G = gridDim.x;

    const int mask = a.g.bps == 2 ? 0xffff : 0xff;
    MomentBlockAcc acc;
    EncStats st;   // (enc_transform's parameter; unused with STATS = false)
    EncUnit<VW> u;
    DecRaw<SUB, VW> given;
    int m = blockIdx.x, s = 0;
    {
        const int t = map_subtile(a.m, a.e.g, m, 0);
        enc_load<VW, IN16>(u, a.e, t, tx, ty, NW);
        dec_issue<SUB, VW>(given, a.g, t, tx, ty, NW);
    }
    while (m < a.m.totalMapTiles) {   // workgroup-uniform
        if (u.valid) {
            float c0[2 * VW], c1[2 * VW], c2[2 * VW];
            enc_transform<CS, VW, LM == 5 || LM == 6, LM == 6, false>(u, a.e, fr.k, c0, c1, c2, st, fr.s_half);
            const MomentMeasureUnit<SUB, VW> out{given, a.g, acc, mask};
            enc_codes<CS, SUB, VW, LM == 6 ? 5 : LM>(c0, c1, c2, a.e.q, static_cast<const float *>(nullptr), fr.s_rec, out);   // (record searches: no table pointer)
        }
        const bool last = s + 1 == a.m.S;
        const int mn = last ? m + G : m, sn = last ? 0 : s + 1;
        const int t = map_subtile(a.m, a.e.g, mn, sn);
        enc_load<VW, IN16>(u, a.e, t, tx, ty, NW);
        dec_issue<SUB, VW>(given, a.g, t, tx, ty, NW);
        if (last) {
            dist_map_flush<VW>(acc, s_map, a.m, a.e.g, a.map, m, tx);
            acc.reset();
        }
        m = mn;
        s = sn;
    }
}

// ---- TRANSCODE DISTORTION MAP -----------------------------------------------------------------------
// k_transcode_distortion's four words per plane for every B x B block of luma pixels of the TARGET (a 4:2:0 target plane: the
// samples co-sited with them; the source's subsampling plays no part): k_transcode_distortion's front end and launch bound,
// k_distortion_map's accumulation, owner per word and loop -- the next source unit and, right behind it, the next given words are
// issued before the flush and are in flight across its barriers.  Reads 3 + 3 B per pixel (profile 2 on both sides), writes 96 B
// per block; no float frame, no scratch planes, no global atomic, no memset.
struct TransDistMapArgs {
    DecArgs d;         // the source planes, as TransArgs::d
    EncArgs e;         // the target quantizer, as TransDistArgs::e
    DecArgs g;         // the given planes, as TransDistArgs::g
    uint64_t *map;     // as MapArgs::map
    MapGeom m;
};

template <int CSD, bool SUBD, int CSE, bool SUBE, int VW, int LM>
__global__ __launch_bounds__((TransDistBound<CSD, CSE>::value)) void k_transcode_distortion_map(const TransDistMapArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned long long *const s_map = dist_map_words();
    using Front = PlaneFront<CSD, CSE, LM>;
    stage_tables<Front::WHAT_D, Front::WHAT_E>(smem, a.d.q, a.e.q);
    constexpr int off = lds_table_offset<Front::WHAT_D | Front::WHAT_E>();
    const float *s_lut = reinterpret_cast<const float *>(smem + off);
    const float *s_uv = reinterpret_cast<const float *>(smem + off + lds_lut_bytes(a.d.q));   // u'v' table, or y table + chroma terms
    const uint32_t *s_rec = reinterpret_cast<const uint32_t *>(smem + off + lds_quant_bytes<Front::WHAT_D>(a.d.q));
    const PowfTablesWide *pw = reinterpret_cast<const PowfTablesWide *>(smem);
    const XformConst kd = make_xform_const<CSD>(a.d.sc, a.d.q.Lmax, pw);
    const XformConst ke = make_xform_const<CSE>(a.e.sc, a.e.q.Lmax, pw);

    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int NW = blockDim.x >> 6;
    const int G = gridDim.x;

    const int mask = a.g.bps == 2 ? 0xffff : 0xff;
    DistBlockAcc acc;
    EncStats st;   // (enc_transform's parameter; unused with STATS = false)
    DecUnit<SUBD, VW> cur, nxt;
    DecRaw<SUBE, VW> given;
    int m = blockIdx.x, s = 0;
    {
        const int t = map_subtile(a.m, a.d.g, m, 0);
        dec_load<SUBD, VW>(cur, a.d, t, tx, ty, NW);
        dec_issue<SUBE, VW>(given, a.g, t, tx, ty, NW);
    }
    while (m < a.m.totalMapTiles) {   // workgroup-uniform
        if (cur.valid) {
            EncUnit<VW> u;
            if constexpr (Front::YD) {
                // two copies of the decode arithmetic, chosen by a kernel argument, as in k_decode
                if (kd.sc_mode == 1)
                    dec_values<CSD, SUBD, VW, false, true, true>(cur, a.d, kd, s_lut, s_uv, u.in);
                else
                    dec_values<CSD, SUBD, VW, false, true, false>(cur, a.d, kd, s_lut, s_uv, u.in);
            } else {
                dec_values<CSD, SUBD, VW, true>(cur, a.d, kd, s_lut, s_uv, u.in);
            }
            float c0[2 * VW], c1[2 * VW], c2[2 * VW];
            enc_transform<CSE, VW, Front::YE, false, false>(u, a.e, ke, c0, c1, c2, st);
            const DistMeasureUnit<SUBE, VW, DistBlockAcc> out{given, a.g, acc, mask};
            enc_codes<CSE, SUBE, VW, LM>(c0, c1, c2, a.e.q, static_cast<const float *>(nullptr), s_rec, out);   // (record searches: no table pointer)
        }
        const bool last = s + 1 == a.m.S;
        const int mn = last ? m + G : m, sn = last ? 0 : s + 1;
        const int t = map_subtile(a.m, a.d.g, mn, sn);
        dec_load<SUBD, VW>(nxt, a.d, t, tx, ty, NW);
        dec_issue<SUBE, VW>(given, a.g, t, tx, ty, NW);
        if (last) {
            dist_map_flush<VW>(acc, s_map, a.m, a.d.g, a.map, m, tx);
            acc.reset();
        }
        cur = nxt;
        m = mn;
        s = sn;
    }
}

// ---- TRANSCODE MOMENTS MAP --------------------------------------------------------------------------
// k_moments_map's five sums per plane for every B x B block of luma pixels of the TARGET (B = 8, 16, 32 or 64), e what k_transcode
// would store for the source planes and g the given sample: k_transcode_distortion_map with the consumer (MomentMeasureUnit) and
// the record (MomentBlockAcc) changed, everything else as written out there -- argument struct included (TransDistMapArgs; map:
// 15 words per block).  Reads 3 + 3 B per pixel (profile 2 on both sides), writes 120 B per block; no float frame, no scratch
// planes, no global atomic, no memset.
// Register budget (profiles/transcode_moments_map_codegen.txt has the compiler's table): the record is 24 registers against
// DistBlockAcc's 15.  The Lu'v' -> Lu'v' kernels at VW 4 sit at 120 - 128 registers in k_transcode_distortion_map, some with scratch
// already: they are allocated for three waves per SIMD (168 registers) in workgroups of at most 512 threads, as the moments_wide
// kernels of k_moments_map.  The Lu'v' -> Lu'v' kernels at VW 2 keep 1024 threads and four waves (128 registers), the pairs with YCbCr
// TransDistBound's 512 threads, which leaves them two waves per SIMD (256 registers).  transcode_plan clamps the launch to
// transmoments_threads_bound: a launch never exceeds what its kernel was compiled for.
constexpr bool transmoments_any_y(int csd, int cse) { return csd == CS_YCBCR || cse == CS_YCBCR; }
constexpr int transmoments_threads_bound(int csd, int cse, int vw) { return (transmoments_any_y(csd, cse) || vw == 4) ? 512 : 1024; }
constexpr int transmoments_waves(int csd, int cse, int vw) { return transmoments_any_y(csd, cse) ? 2 : vw == 4 ? 3 : 4; }

template <int CSD, bool SUBD, int CSE, bool SUBE, int VW, int LM>
__global__ __launch_bounds__(transmoments_threads_bound(CSD, CSE, VW)) __attribute__((amdgpu_waves_per_eu(transmoments_waves(CSD, CSE, VW))))
void k_transcode_moments_map(const TransDistMapArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned long long *const s_map = dist_map_words<MomentBlockAcc>();
    using Front = PlaneFront<CSD, CSE, LM>;
    stage_tables<Front::WHAT_D, Front::WHAT_E>(smem, a.d.q, a.e.q);
    constexpr int off = lds_table_offset<Front::WHAT_D | Front::WHAT_E>();
    const float *s_lut = reinterpret_cast<const float *>(smem + off);
    const float *s_uv = reinterpret_cast<const float *>(smem + off + lds_lut_bytes(a.d.q));   // u'v' table, or y table + chroma terms
    const uint32_t *s_rec = reinterpret_cast<const uint32_t *>(smem + off + lds_quant_bytes<Front::WHAT_D>(a.d.q));
    const PowfTablesWide *pw = reinterpret_cast<const PowfTablesWide *>(smem);
    const XformConst kd = make_xform_const<CSD>(a.d.sc, a.d.q.Lmax, pw);
    const XformConst ke = make_xform_const<CSE>(a.e.sc, a.e.q.Lmax, pw);

    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int NW = blockDim.x >> 6;
    const int G = gridDim.x;

    const int mask = a.g.bps == 2 ? 0xffff : 0xff;
    MomentBlockAcc acc;
    EncStats st;   // (enc_transform's parameter; unused with STATS = false)
    DecUnit<SUBD, VW> cur, nxt;
    DecRaw<SUBE, VW> given;
    int m = blockIdx.x, s = 0;
    {
        const int t = map_subtile(a.m, a.d.g, m, 0);
        dec_load<SUBD, VW>(cur, a.d, t, tx, ty, NW);
        dec_issue<SUBE, VW>(given, a.g, t, tx, ty, NW);
    }
    while (m < a.m.totalMapTiles) {   // workgroup-uniform
        if (cur.valid) {
            EncUnit<VW> u;
            if constexpr (Front::YD) {
                // two copies of the decode arithmetic, chosen by a kernel argument, as in k_decode
                if (kd.sc_mode == 1)
                    dec_values<CSD, SUBD, VW, false, true, true>(cur, a.d, kd, s_lut, s_uv, u.in);
                else
                    dec_values<CSD, SUBD, VW, false, true, false>(cur, a.d, kd, s_lut, s_uv, u.in);
            } else {
                dec_values<CSD, SUBD, VW, true>(cur, a.d, kd, s_lut, s_uv, u.in);
            }
            float c0[2 * VW], c1[2 * VW], c2[2 * VW];
            enc_transform<CSE, VW, Front::YE, false, false>(u, a.e, ke, c0, c1, c2, st);
            const MomentMeasureUnit<SUBE, VW> out{given, a.g, acc, mask};
            enc_codes<CSE, SUBE, VW, LM>(c0, c1, c2, a.e.q, static_cast<const float *>(nullptr), s_rec, out);   // (record searches: no table pointer)
        }
        const bool last = s + 1 == a.m.S;
        const int mn = last ? m + G : m, sn = last ? 0 : s + 1;
        const int t = map_subtile(a.m, a.d.g, mn, sn);
        dec_load<SUBD, VW>(nxt, a.d, t, tx, ty, NW);
        dec_issue<SUBE, VW>(given, a.g, t, tx, ty, NW);
        if (last) {
            dist_map_flush<VW>(acc, s_map, a.m, a.d.g, a.map, m, tx);
            acc.reset();
        }
        cur = nxt;
        m = mn;
        s = sn;
    }
}

// ---- HALF-RESOLUTION TRANSCODE DISTORTION, PER FRAME AND PER BLOCK ----------------------------------
// How far GIVEN code planes of (w/2) x (h/2) are from the planes k_transcode_half would write for source planes of w x h: e is the
// sample that kernel stores (the decoded floats, the 2x2 box ((a + b) + (c + d)) * 0.25f, the target's encode), g the sample that is
// there.  k_transcode_half's front end (half_locate / half_issue / half_fill over the TARGET's tiles, a.e.g; a.d.g is the source's
// geometry) with k_transcode_distortion's consumer and flush site, and with k_transcode_distortion_map's loop and owner per word.
// The argument structs are those kernels' (TransDistArgs, TransDistMapArgs); a.g carries the target's geometry (a.g.g == a.e.g), so
// dec_issue finds the given unit of a target tile as it finds any unit, and the given words are issued right behind half_issue's
// loads for the next target unit.  Reads 4 x 3 + 3 B per target pixel at profile 2 on both sides; no scratch planes, no float frame.
// Register budget (profiles/transcode_half_distortion_codegen.txt has the compiler's table): k_transcode_half's kernels plus the
// consumer's accumulators (18 registers per frame, 15 per block) and up to 8 given words.  One function of (CSD, CSE, VW) per
// kernel, which its __launch_bounds__ / amdgpu_waves_per_eu are written with and transcode_plan clamps the launch to.  Every kernel
// is bounded at 512 threads; YCbCr on either side gets two waves per SIMD (256 registers), Lu'v' -> Lu'v' three (168).  Under that
// bound a YCbCr 4:4:4 source (88 - 148 B of scratch per lane at 256 registers) and a Lu'v' 4:4:4 source with a Lu'v' target (148 -
// 232 B at 168) cannot be had at VW 4 without scratch: transhalfdist_vw4 says which families exist at VW 4, the plan asks it, and
// the others are instantiated at VW 2 only.
constexpr int transhalfdist_threads_bound(int csd, int cse, int vw) { return 512; }
constexpr int transhalfdist_waves(int csd, int cse, int vw) { return (csd == CS_YCBCR || cse == CS_YCBCR) ? 2 : 3; }
constexpr int transhalfmap_threads_bound(int csd, int cse, int vw) { return transhalfdist_threads_bound(csd, cse, vw); }
constexpr int transhalfmap_waves(int csd, int cse, int vw) { return transhalfdist_waves(csd, cse, vw); }
// whether the kernels of source (csd, subd) and target colour space cse exist at VW 4 (both calls decide alike: the front end is
// what fills the registers)
constexpr bool transhalfdist_vw4(int csd, bool subd, int cse) { return subd || (csd == CS_LUV && cse == CS_YCBCR); }

template <int CSD, bool SUBD, int CSE, bool SUBE, int VW, int LM>
__global__ __launch_bounds__(transhalfdist_threads_bound(CSD, CSE, VW)) __attribute__((amdgpu_waves_per_eu(transhalfdist_waves(CSD, CSE, VW))))
void k_transcode_half_distortion(const TransDistArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned long long *const s_acc = dist_words();
    using Front = PlaneFront<CSD, CSE, LM>;
    stage_tables<Front::WHAT_D, Front::WHAT_E>(smem, a.d.q, a.e.q);
    constexpr int off = lds_table_offset<Front::WHAT_D | Front::WHAT_E>();
    const float *s_lut = reinterpret_cast<const float *>(smem + off);
    const float *s_uv = reinterpret_cast<const float *>(smem + off + lds_lut_bytes(a.d.q));   // u'v' table, or y table + chroma terms
    const uint32_t *s_rec = reinterpret_cast<const uint32_t *>(smem + off + lds_quant_bytes<Front::WHAT_D>(a.d.q));
    const PowfTablesWide *pw = reinterpret_cast<const PowfTablesWide *>(smem);
    const XformConst kd = make_xform_const<CSD>(a.d.sc, a.d.q.Lmax, pw);
    const XformConst ke = make_xform_const<CSE>(a.e.sc, a.e.q.Lmax, pw);

    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int NW = blockDim.x >> 6;
    const int G = gridDim.x;
    constexpr int NPF = half_prefetch<SUBD, VW>();

    const int mask = a.g.bps == 2 ? 0xffff : 0xff;
    DistAcc acc;
    EncStats st;   // (enc_transform's parameter; unused with STATS = false)
    DecUnit<SUBD, VW> pf[NPF];
    DecRaw<SUBE, VW> given;
    int f = 0, ux = 0, uy = 0;
    bool valid = half_locate(a.e.g, blockIdx.x, tx, ty, NW, f, ux, uy);
    if (valid)
        half_issue<SUBD, VW>(pf, a.d, f, ux, uy);
    dec_issue<SUBE, VW>(given, a.g, blockIdx.x, tx, ty, NW);
    for (int t = blockIdx.x;; t += G) {
        const bool done = t >= a.e.g.totalTiles;
        dist_flush(acc, s_acc, done ? -2 : t / a.e.g.tilesPerFrame, a.out);
        if (done)
            break;
        if (valid) {
            EncUnit<VW> u;
            if constexpr (Front::YD) {
                // two copies of the decode arithmetic, chosen by a kernel argument, as in k_decode
                if (kd.sc_mode == 1)
                    half_fill<CSD, SUBD, VW, false, true, true>(u, pf, a.d, kd, s_lut, s_uv, f, ux, uy);
                else
                    half_fill<CSD, SUBD, VW, false, true, false>(u, pf, a.d, kd, s_lut, s_uv, f, ux, uy);
            } else {
                half_fill<CSD, SUBD, VW, true, false, false>(u, pf, a.d, kd, s_lut, s_uv, f, ux, uy);
            }
            float c0[2 * VW], c1[2 * VW], c2[2 * VW];
            enc_transform<CSE, VW, Front::YE, false, false>(u, a.e, ke, c0, c1, c2, st);
            const DistMeasureUnit<SUBE, VW> out{given, a.g, acc, mask};
            enc_codes<CSE, SUBE, VW, LM>(c0, c1, c2, a.e.q, static_cast<const float *>(nullptr), s_rec, out);   // (record searches: no table pointer)
        }
        valid = half_locate(a.e.g, t + G, tx, ty, NW, f, ux, uy);
        if (valid)
            half_issue<SUBD, VW>(pf, a.d, f, ux, uy);
        dec_issue<SUBE, VW>(given, a.g, t + G, tx, ty, NW);
    }
}

// MapGeom is of the target's geometry; map_subtile names the next target tile, whose source units and, right behind them, given
// words are issued before the flush and are in flight across its barriers
template <int CSD, bool SUBD, int CSE, bool SUBE, int VW, int LM>
__global__ __launch_bounds__(transhalfmap_threads_bound(CSD, CSE, VW)) __attribute__((amdgpu_waves_per_eu(transhalfmap_waves(CSD, CSE, VW))))
void k_transcode_half_distortion_map(const TransDistMapArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned long long *const s_map = dist_map_words();
    using Front = PlaneFront<CSD, CSE, LM>;
    stage_tables<Front::WHAT_D, Front::WHAT_E>(smem, a.d.q, a.e.q);
    constexpr int off = lds_table_offset<Front::WHAT_D | Front::WHAT_E>();
    const float *s_lut = reinterpret_cast<const float *>(smem + off);
    const float *s_uv = reinterpret_cast<const float *>(smem + off + lds_lut_bytes(a.d.q));   // u'v' table, or y table + chroma terms
    const uint32_t *s_rec = reinterpret_cast<const uint32_t *>(smem + off + lds_quant_bytes<Front::WHAT_D>(a.d.q));
    const PowfTablesWide *pw = reinterpret_cast<const PowfTablesWide *>(smem);
    const XformConst kd = make_xform_const<CSD>(a.d.sc, a.d.q.Lmax, pw);
    const XformConst ke = make_xform_const<CSE>(a.e.sc, a.e.q.Lmax, pw);

    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int NW = blockDim.x >> 6;
    const int G = gridDim.x;
    constexpr int NPF = half_prefetch<SUBD, VW>();

    const int mask = a.g.bps == 2 ? 0xffff : 0xff;
    DistBlockAcc acc;
    EncStats st;   // (enc_transform's parameter; unused with STATS = false)
    DecUnit<SUBD, VW> pf[NPF];
    DecRaw<SUBE, VW> given;
    int m = blockIdx.x, s = 0;
    int f = 0, ux = 0, uy = 0;
    bool valid;
    {
        const int t = map_subtile(a.m, a.e.g, m, 0);
        valid = half_locate(a.e.g, t, tx, ty, NW, f, ux, uy);
        if (valid)
            half_issue<SUBD, VW>(pf, a.d, f, ux, uy);
        dec_issue<SUBE, VW>(given, a.g, t, tx, ty, NW);
    }
    while (m < a.m.totalMapTiles) {   // workgroup-uniform
        if (valid) {
            EncUnit<VW> u;
            if constexpr (Front::YD) {
                // two copies of the decode arithmetic, chosen by a kernel argument, as in k_decode
                if (kd.sc_mode == 1)
                    half_fill<CSD, SUBD, VW, false, true, true>(u, pf, a.d, kd, s_lut, s_uv, f, ux, uy);
                else
                    half_fill<CSD, SUBD, VW, false, true, false>(u, pf, a.d, kd, s_lut, s_uv, f, ux, uy);
            } else {
                half_fill<CSD, SUBD, VW, true, false, false>(u, pf, a.d, kd, s_lut, s_uv, f, ux, uy);
            }
            float c0[2 * VW], c1[2 * VW], c2[2 * VW];
            enc_transform<CSE, VW, Front::YE, false, false>(u, a.e, ke, c0, c1, c2, st);
            const DistMeasureUnit<SUBE, VW, DistBlockAcc> out{given, a.g, acc, mask};
            enc_codes<CSE, SUBE, VW, LM>(c0, c1, c2, a.e.q, static_cast<const float *>(nullptr), s_rec, out);   // (record searches: no table pointer)
        }
        const bool last = s + 1 == a.m.S;
        const int mn = last ? m + G : m, sn = last ? 0 : s + 1;
        const int t = map_subtile(a.m, a.e.g, mn, sn);
        valid = half_locate(a.e.g, t, tx, ty, NW, f, ux, uy);
        if (valid)
            half_issue<SUBD, VW>(pf, a.d, f, ux, uy);
        dec_issue<SUBE, VW>(given, a.g, t, tx, ty, NW);
        if (last) {
            dist_map_flush<VW>(acc, s_map, a.m, a.e.g, a.map, m, tx);
            acc.reset();
        }
        m = mn;
        s = sn;
    }
}

// ---- PLANES IN, AS THEY ARE -------------------------------------------------------------------------
// The third front end over the same three consumers: e is not computed, it is the sample present in a plane set A, as g is the one
// present in a set B -- both read as the decoder reads them, no quantizer on either side (DecArgs::q stays unused), no tables, no
// dynamic LDS, no transform, no search.  Reads 3 + 3 B per pixel at profile 2.  With no arithmetic to hide them behind, the loads are
// these kernels' limit -- their latency, not their bytes: 0.18 - 0.42 of the HBM rate as measured, profile 0 no faster than profile 2
// (DESIGN.md 3.13 has the counters and the open point).
//   k_planes_distortion        DistMeasureUnit<., ., DistAcc>,       dist_words / dist_flush,               k_distortion's loop
//   k_planes_distortion_map    DistMeasureUnit<., ., DistBlockAcc>,  dist_map_words / dist_map_flush,       k_distortion_map's loop
//   k_planes_moments_map       MomentMeasureUnit,                    dist_map_words<MomentBlockAcc> / ...,  k_distortion_map's loop
// Both sets' words are fetched by dec_issue one iteration ahead, A's right in front of B's; A's rows are unpacked where they are
// consumed (given_row: vector words where the set is `aligned`, load_samples byte by byte where it is not, decided per set) and
// handed over in enc_codes' order.  The consumers' mask is a no-op on unpacked samples.
struct PlanesMeasureArgs {
    DecArgs a;         // set A (e): g, src, stride, src_frame_stride, bps, aligned
    DecArgs g;         // set B (g): the same geometry and sample size, its own pointers, strides and `aligned`
    uint64_t *out;     // DistArgs::out (zeroed before the launch), or MapArgs::map (needs no zeroing)
    MapGeom m;         // the map kernels only
};

// the rows of unit `e` of set A to the consumer, in enc_codes' order
template <bool SUB, int VW, typename Out>
LH_DEV void planes_rows(const DecRaw<SUB, VW> &e, const DecArgs &a, const Out &out)
{
#pragma unroll
    for (int r = 0; r < 2; r++) {
        int row[VW];
        given_row<SUB, VW, VW>(e, a, 0, r, row);
        out.template row<VW>(0, r, row);
    }
    if constexpr (SUB) {
        constexpr int NQ = VW / 2;
        int k1[NQ], k2[NQ];
        given_row<SUB, VW, NQ>(e, a, 1, 0, k1);
        given_row<SUB, VW, NQ>(e, a, 2, 0, k2);
        out.template row<NQ>(1, 0, k1);
        out.template row<NQ>(2, 0, k2);
    } else {
#pragma unroll
        for (int pl = 1; pl < 3; pl++) {
#pragma unroll
            for (int r = 0; r < 2; r++) {
                int row[VW];
                given_row<SUB, VW, VW>(e, a, pl, r, row);
                out.template row<VW>(pl, r, row);
            }
        }
    }
}

// Register budget (profiles/planes_measure_codegen.txt has the compiler's table): the accumulators (15 - 24 registers) and the raw
// words of both sets; every variant fits the 128 registers of a 1024-thread workgroup without scratch, so the bound stays there and
// no waves-per-SIMD target is asked for.
constexpr int PLANES_MEASURE_BOUND = 1024;

template <bool SUB, int VW>
__global__ __launch_bounds__(PLANES_MEASURE_BOUND) void k_planes_distortion(const PlanesMeasureArgs a)
{
    unsigned long long *const s_acc = dist_words();
    __syncthreads();   // (no stage_tables behind the zeroing here)

    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int NW = blockDim.x >> 6;
    const int G = gridDim.x;

    const int mask = a.g.bps == 2 ? 0xffff : 0xff;
    DistAcc acc;
    DecRaw<SUB, VW> e, given;
    dec_issue<SUB, VW>(e, a.a, blockIdx.x, tx, ty, NW);
    dec_issue<SUB, VW>(given, a.g, blockIdx.x, tx, ty, NW);
    for (int t = blockIdx.x;; t += G) {
        const bool done = t >= a.a.g.totalTiles;        // workgroup-uniform, as the frame index is
        dist_flush(acc, s_acc, done ? -2 : t / a.a.g.tilesPerFrame, a.out);
        if (done)
            break;
        if (e.valid) {
            const DistMeasureUnit<SUB, VW> out{given, a.g, acc, mask};
            planes_rows<SUB, VW>(e, a.a, out);
        }
        dec_issue<SUB, VW>(e, a.a, t + G, tx, ty, NW);
        dec_issue<SUB, VW>(given, a.g, t + G, tx, ty, NW);
    }
}

// the loop of both map kernels: k_distortion_map's, the next sub-tile's loads issued before the flush
template <bool SUB, int VW, typename Acc, typename Unit>
LH_DEV void planes_map_loop(const PlanesMeasureArgs &a, unsigned long long *s_map)
{
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int NW = blockDim.x >> 6;
    const int G = gridDim.x;

    const int mask = a.g.bps == 2 ? 0xffff : 0xff;
    Acc acc;
    DecRaw<SUB, VW> e, given;
    int m = blockIdx.x, s = 0;
    {
        const int t = map_subtile(a.m, a.a.g, m, 0);
        dec_issue<SUB, VW>(e, a.a, t, tx, ty, NW);
        dec_issue<SUB, VW>(given, a.g, t, tx, ty, NW);
    }
    while (m < a.m.totalMapTiles) {   // workgroup-uniform
        if (e.valid) {
            const Unit out{given, a.g, acc, mask};
            planes_rows<SUB, VW>(e, a.a, out);
        }
        const bool last = s + 1 == a.m.S;
        const int mn = last ? m + G : m, sn = last ? 0 : s + 1;
        const int t = map_subtile(a.m, a.a.g, mn, sn);
        dec_issue<SUB, VW>(e, a.a, t, tx, ty, NW);
        dec_issue<SUB, VW>(given, a.g, t, tx, ty, NW);
        if (last) {
            dist_map_flush<VW>(acc, s_map, a.m, a.a.g, a.out, m, tx);
            acc.reset();
        }
        m = mn;
        s = sn;
    }
}

template <bool SUB, int VW>
__global__ __launch_bounds__(PLANES_MEASURE_BOUND) void k_planes_distortion_map(const PlanesMeasureArgs a)
{
    unsigned long long *const s_map = dist_map_words();
    __syncthreads();
    planes_map_loop<SUB, VW, DistBlockAcc, DistMeasureUnit<SUB, VW, DistBlockAcc>>(a, s_map);
}

template <bool SUB, int VW>
__global__ __launch_bounds__(PLANES_MEASURE_BOUND) void k_planes_moments_map(const PlanesMeasureArgs a)
{
    unsigned long long *const s_map = dist_map_words<MomentBlockAcc>();
    __syncthreads();
    planes_map_loop<SUB, VW, MomentBlockAcc, MomentMeasureUnit<SUB, VW>>(a, s_map);
}

// ---- CONTENT LIGHT LEVEL ----------------------------------------------------------------------------
// A fourth consumer, which needs neither enc_codes nor given planes: what an HDR10 deliverable states about its own content, per
// frame, over m = max(R, G, B) (MaxCLL / MaxFALL) and over the luminance y = rgb_to_xyz's Y row without clamp_xyz, both after
// `* scale` (the stream's preScaling gives cd/m2) and in units of 1/256 (include/lumahip_compare.h has the normative text):
//   out[f * 8 + .] = { sum q(m), max q(m), #(m * 256 >= 2^32), #(m NaN), sum q(y), max q(y), #(y * 256 >= 2^32), #(y NaN) }
// Two front ends: the frames themselves (k_light_level: enc_load, float or binary16; 12 / 6 B per pixel read, nothing written) and
// code planes (k_planes_light_level: dec_load + dec_values under the context's quantizer, i.e. exactly the floats the decode
// kernels would store; 3 B per pixel at profile 2).  Integers throughout: the words do not depend on the launch shape or on the
// order of arrival.
constexpr int LIGHT_WORDS = 8;

// q: a non-negative value in units of 1/256 as an unsigned 32-bit integer.  The three cases are written out as selects (no branch
// per pixel), and the conversion only ever sees a value inside its range
LH_DEV uint32_t light_q(float v, uint32_t &over)
{
    const float t = v * 256.0f;
    const bool positive = t > 0.0f;              // false for NaN, negatives, both zeros, -inf
    const bool big = t >= 4294967296.0f;
    over += big;
    const uint32_t fl = (uint32_t)((positive && !big) ? t : 0.0f);   // 0 <= . < 2^32: the conversion truncates, which is the floor
    return big ? 0xFFFFFFFFu : fl;
}

// the larger of two floats, a NaN ignored: fmaxf
LH_DEV float light_max(float a, float b) { return fmaxf(a, b); }

struct LightAcc {
    uint64_t sum[2];               // [0] of q(m), [1] of q(y)
    uint32_t mx[2], over[2], nan[2];   // (a lane's share of one frame is far below 2^32 pixels)
    int frame = -1;                // no frame yet
    LH_DEVS LightAcc() { reset(); }
    LH_DEVS void reset()
    {
        sum[0] = sum[1] = 0;
        mx[0] = mx[1] = over[0] = over[1] = nan[0] = nan[1] = 0;
    }
};

// the consumer: a unit's floats in the layout of EncUnit::in
template <int VW>
struct LightUnit {
    LightAcc &acc;
    float scale;
    LH_DEVS void take(const float (&in)[3][2][VW]) const
    {
#pragma unroll
        for (int r = 0; r < 2; r++)
#pragma unroll
            for (int i = 0; i < VW; i++) {
                float R = in[0][r][i], G = in[1][r][i], B = in[2][r][i];
                if (scale != 1.0f) {   // (kernel argument: uniform; x * 1.0f == x)
                    R *= scale;
                    G *= scale;
                    B *= scale;
                }
                const float m = light_max(light_max(R, G), B);
                const float y = (0.212656f * R + 0.715158f * G) + 0.072186f * B;
                const uint32_t qm = light_q(m, acc.over[0]), qy = light_q(y, acc.over[1]);
                acc.sum[0] += qm;
                acc.sum[1] += qy;
                acc.mx[0] = qm > acc.mx[0] ? qm : acc.mx[0];
                acc.mx[1] = qy > acc.mx[1] ? qy : acc.mx[1];
                acc.nan[0] += m != m;
                acc.nan[1] += y != y;
            }
    }
};

// The 8 words of LDS in which the waves of a light-level workgroup meet, zeroed: called before the front end's stage_tables (or a
// barrier of the kernel's own).  Must stay LH_DEV, as dist_words
LH_DEV unsigned long long *light_words()
{
    __shared__ unsigned long long s_acc[LIGHT_WORDS];
    if (threadIdx.x < LIGHT_WORDS)
        s_acc[threadIdx.x] = 0;
    return s_acc;
}

// one step of the meeting of a wave's lanes (map_lanes_step's, for LightAcc)
template <typename Xch>
LH_DEV void light_lanes_step(LightAcc &acc, Xch xch)
{
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const uint32_t lo = xch((uint32_t)acc.sum[k]), hi = xch((uint32_t)(acc.sum[k] >> 32));
        acc.sum[k] += ((uint64_t)hi << 32) | lo;
        const uint32_t m = xch(acc.mx[k]);
        acc.mx[k] = m > acc.mx[k] ? m : acc.mx[k];
        acc.over[k] += xch(acc.over[k]);
        acc.nan[k] += xch(acc.nan[k]);
    }
}

// dist_flush's pattern: the one flush site of a light-level loop, called by every thread of the workgroup at the top of every
// iteration with f = the frame of the iteration's tile, or -2 past the last tile.  When the frame changes, the 32 lanes of each half
// of a wave add up among themselves (DPP and one swizzle, as map_lanes_meet: every lane has something to add here, and 256 lanes on
// 8 LDS words would serialise), lanes 0 and 32 add into the 8 words of LDS, and one thread per word hands it to out[frame * 8 + .]
// -- one 64-bit global atomic per workgroup, frame and word -- and clears it.
LH_DEV void light_flush(LightAcc &acc, unsigned long long *s_acc, int f, uint64_t *out)
{
    if (f != acc.frame) {
        if (acc.frame >= 0) {
            light_lanes_step(acc, [](uint32_t v) { return dpp_lane<0xb1>(v); });    // quad_perm [1, 0, 3, 2]
            light_lanes_step(acc, [](uint32_t v) { return dpp_lane<0x4e>(v); });    // quad_perm [2, 3, 0, 1]
            light_lanes_step(acc, [](uint32_t v) { return dpp_lane<0x141>(v); });   // row_half_mirror
            light_lanes_step(acc, [](uint32_t v) { return dpp_lane<0x140>(v); });   // row_mirror
            light_lanes_step(acc, [](uint32_t v) { return swz16_lane(v); });        // the other row of 32
            if ((threadIdx.x & 31) == 0) {
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    atomicAdd(&s_acc[4 * k + 0], (unsigned long long)acc.sum[k]);
                    atomicMax(&s_acc[4 * k + 1], (unsigned long long)acc.mx[k]);
                    atomicAdd(&s_acc[4 * k + 2], (unsigned long long)acc.over[k]);
                    atomicAdd(&s_acc[4 * k + 3], (unsigned long long)acc.nan[k]);
                }
            }
            __syncthreads();
            if (threadIdx.x < LIGHT_WORDS) {
                const unsigned long long v = s_acc[threadIdx.x];
                s_acc[threadIdx.x] = 0;
                unsigned long long *dst = reinterpret_cast<unsigned long long *>(out) + (size_t)acc.frame * LIGHT_WORDS + threadIdx.x;
                if (v != 0) {
                    if ((threadIdx.x & 3) == 1)
                        atomicMax(dst, v);
                    else
                        atomicAdd(dst, v);
                }
            }
            __syncthreads();
        }
        acc.reset();
        acc.frame = f;
    }
}

struct LightArgs {
    EncArgs e;       // g, src, frame_stride of the frames; everything else unused (no quantizer, no tables)
    float scale;
    uint64_t *out;   // [nframes][LIGHT_WORDS], zeroed before the launch
};

// Register budget: two units in flight (2 x 24 floats at VW 4) and the accumulators (10); every variant fits the 128 registers of
// a 1024-thread workgroup (profiles/light_level_codegen.txt has the compiler's table).
constexpr int LIGHT_BOUND = 1024;

// The kernel has no arithmetic to speak of and no stores behind which a single-buffered load could hide (what that costs the
// plane-to-plane kernels: DESIGN.md 3.13), so it holds TWO units: the loads of tile t + G are issued before unit t is consumed,
// and the wait in front of unit t leaves them in flight.  The two units take turns -- `step` is called with them one way
// round, then the other -- so that neither is ever copied (a copy would wait for its loads); the flush stays one site, in `step`.
template <int VW, bool IN16>
__global__ __launch_bounds__(LIGHT_BOUND) void k_light_level(const LightArgs a)
{
    unsigned long long *const s_acc = light_words();
    __syncthreads();   // (no stage_tables behind the zeroing here)

    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int NW = blockDim.x >> 6;
    const int G = gridDim.x;

    LightAcc acc;
    const LightUnit<VW> unit{acc, a.scale};
    EncUnit<VW> u0, u1;
    int t = blockIdx.x;
    // tile t is in `cur`; false past the last tile
    const auto step = [&](EncUnit<VW> &cur, EncUnit<VW> &nxt) {
        const bool done = t >= a.e.g.totalTiles;        // workgroup-uniform, as the frame index is
        light_flush(acc, s_acc, done ? -2 : t / a.e.g.tilesPerFrame, a.out);
        if (done)
            return false;
        enc_load<VW, IN16>(nxt, a.e, t + G, tx, ty, NW);
        if (cur.valid)
            unit.take(cur.in);
        t += G;
        return true;
    };
    enc_load<VW, IN16>(u0, a.e, t, tx, ty, NW);
    while (step(u0, u1) && step(u1, u0)) {
    }
}

struct PlanesLightArgs {
    DecArgs d;       // q, g, src, stride, src_frame_stride, sc, bps, aligned of the planes, as TransArgs::d under the context's quantizer
    float scale;
    uint64_t *out;   // LightArgs::out
};

// what stage_tables stages for the planes' quantizer: the decode kernels' tables in LDS (transfer function and chroma depth up to 12 bits)
template <int CS>
struct LightFront {
    static constexpr bool Y = CS == CS_YCBCR;
    static constexpr int WHAT = STAGE_LUT | (Y ? STAGE_POWF | STAGE_YT | STAGE_CT : CS == CS_LUV ? STAGE_UV : 0);
    // threads per workgroup the variants are register-allocated for: as TransDistBound, the YCbCr arithmetic wants its 128 registers
    static constexpr int bound = Y ? 512 : 1024;
};

// k_transcode's source-side loop (dec_load of the next unit behind the current one's arithmetic; not tuned here) in front of LightUnit
template <int CS, bool SUB, int VW>
__global__ __launch_bounds__((LightFront<CS>::bound)) void k_planes_light_level(const PlanesLightArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    using Front = LightFront<CS>;
    unsigned long long *const s_acc = light_words();
    stage_tables<Front::WHAT>(smem, a.d.q);
    constexpr int off = lds_table_offset<Front::WHAT>();
    const float *s_lut = reinterpret_cast<const float *>(smem + off);
    const float *s_uv = reinterpret_cast<const float *>(smem + off + lds_lut_bytes(a.d.q));   // u'v' table, or y table + chroma terms
    const XformConst k = make_xform_const<CS>(a.d.sc, a.d.q.Lmax, reinterpret_cast<const PowfTablesWide *>(smem));

    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int NW = blockDim.x >> 6;
    const int G = gridDim.x;

    LightAcc acc;
    const LightUnit<VW> unit{acc, a.scale};
    DecUnit<SUB, VW> cur, nxt;
    dec_load<SUB, VW>(cur, a.d, blockIdx.x, tx, ty, NW);
    for (int t = blockIdx.x;; t += G) {
        const bool done = t >= a.d.g.totalTiles;        // workgroup-uniform, as the frame index is
        light_flush(acc, s_acc, done ? -2 : t / a.d.g.tilesPerFrame, a.out);
        if (done)
            break;
        if (cur.valid) {
            float vals[3][2][VW];
            if constexpr (Front::Y) {
                // two copies of the decode arithmetic, chosen by a kernel argument, as in k_decode
                if (k.sc_mode == 1)
                    dec_values<CS, SUB, VW, false, true, true>(cur, a.d, k, s_lut, s_uv, vals);
                else
                    dec_values<CS, SUB, VW, false, true, false>(cur, a.d, k, s_lut, s_uv, vals);
            } else {
                dec_values<CS, SUB, VW, CS == CS_LUV>(cur, a.d, k, s_lut, s_uv, vals);
            }
            unit.take(vals);
        }
        dec_load<SUB, VW>(nxt, a.d, t + G, tx, ty, NW);
        cur = nxt;
    }
}

// ---- stand-alone colour transform (LumaQuantizer::transformColorSpace as public API) ---------------
struct XfArgs {
    float *buf;
    size_t frame_stride;
    size_t chan_stride;  // w*h
    size_t n2;           // pixel pairs per frame
    int nframes;
    float sc;
    float Lmax;
};

template <int CS, bool FWD>
__global__ __launch_bounds__(256) void k_transform(const XfArgs a)
{
    __shared__ __attribute__((aligned(16))) unsigned char s_raw[CS == CS_YCBCR ? sizeof(PowfTablesWide) : 16];
    PowfTablesWide &s_pw = *reinterpret_cast<PowfTablesWide *>(s_raw);
    if constexpr (CS == CS_YCBCR) {
        stage_powf_tables(&s_pw);
        __syncthreads();
    }
    const XformConst k = make_xform_const<CS>(a.sc, a.Lmax, &s_pw);
    const size_t total = a.n2 * a.nframes;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t f = i / a.n2, j = i - f * a.n2;
        float *p = a.buf + f * a.frame_stride + 2 * j;
        float v0[2], v1[2], v2[2], o0[2], o1[2], o2[2];
        load_px<2>(p, v0);
        load_px<2>(p + a.chan_stride, v1);
        load_px<2>(p + 2 * a.chan_stride, v2);
#pragma unroll
        for (int e = 0; e < 2; e++) {
            if constexpr (FWD) {
                xform_fwd<CS>(v0[e] * k.sc, v1[e] * k.sc, v2[e] * k.sc, k, o0[e], o1[e], o2[e]);
            } else {
                xform_inv<CS>(v0[e], v1[e], v2[e], k, o0[e], o1[e], o2[e]);
                o0[e] = div_ieee(o0[e], k.sc);
                o1[e] = div_ieee(o1[e], k.sc);
                o2[e] = div_ieee(o2[e], k.sc);
            }
        }
        store_px<2>(p, o0);
        store_px<2>(p + a.chan_stride, o1);
        store_px<2>(p + 2 * a.chan_stride, o2);
    }
}

// ---- the reference's mean luminance, exactly ---------------------------------------------------------
// LumaEncoder::setVpxChannel accumulates plane 0 into ONE fp32 variable in raster order (src/luma_encoder.cpp:276,294,314)
// and warns when avg / (w*h) <= 1.  A sequential fp32 sum is not associative: the encode kernels' per-frame statistics
// (tree / atomic order) give a more accurate but different number, typically 1e-4 relative apart at 4K.  When the caller
// needs the reference's value -- the host entry points do when the fast mean is within 1 % of the threshold -- these two
// kernels reproduce it: k_channel0 writes the transformed channel 0 of one frame, k_seq_sum adds it up in the reference's
// order (one wave; lanes load 64 consecutive values at a time, the adds run lane-uniformly in raster order; ~25 ms at 4K).
template <int CS, bool IN16 = false>
__global__ __launch_bounds__(256) void k_channel0(const float *src, size_t chan_stride, size_t n, float sc, float Lmax, float *out)
{
    __shared__ __attribute__((aligned(16))) unsigned char s_raw[CS == CS_YCBCR ? sizeof(PowfTablesWide) : 16];
    PowfTablesWide &s_pw = *reinterpret_cast<PowfTablesWide *>(s_raw);
    if constexpr (CS == CS_YCBCR) {
        stage_powf_tables(&s_pw);
        __syncthreads();
    }
    const XformConst k = make_xform_const<CS>(sc, Lmax, &s_pw);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        float c0, c1, c2;
        float r, g, b;
        if constexpr (IN16) {   // the frame was uploaded as binary16
            const _Float16 *hp = reinterpret_cast<const _Float16 *>(src);
            r = (float)hp[i];
            g = (float)hp[i + chan_stride];
            b = (float)hp[i + 2 * chan_stride];
        } else {
            r = src[i];
            g = src[i + chan_stride];
            b = src[i + 2 * chan_stride];
        }
        xform_fwd<CS>(r * sc, g * sc, b * sc, k, c0, c1, c2);
        out[i] = c0;
    }
}

// Test probe: quantize_lut<LM, 4, NONNEG> -- the instantiation the Lu'v' encode kernels call for a row of four
// luminances -- over consecutive fp32 bit patterns (tests/test_gpu_exhaustive.py; NONNEG promises v >= 0 or NaN, so
// that sweep covers 0 .. 0x7fffffff plus the sign-set NaNs 0xff800001 .. 0xffffffff).
template <int LM, bool NONNEG>
__global__ __launch_bounds__(256) void k_quantize_probe(const QuantDev q, uint16_t *out, uint32_t first_bits, size_t n4)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    stage_tables<(LM == 0 ? STAGE_LUT : 0) | ((LM == 3 || LM == 7) ? STAGE_REC : 0)>(smem, q);
    const float *s_lut = reinterpret_cast<const float *>(smem);
    const uint32_t *s_rec = reinterpret_cast<const uint32_t *>(smem);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        float v[4];
        int c[4];
#pragma unroll
        for (int j = 0; j < 4; j++)
            v[j] = __uint_as_float(first_bits + (uint32_t)(4 * i + j));
        if constexpr (LM == 3 || LM == 7)
            quantize_lut<LM, 4, NONNEG>(v, c, s_lut, s_rec, q);
        else if constexpr (LM == 4)
            quantize_lut<LM, 4, NONNEG>(v, c, q.lut, q.rec, q);
        else if constexpr (LM == 0)
            quantize_lut<LM, 4, NONNEG>(v, c, s_lut, s_rec, q);
        else
            quantize_lut<LM, 4, NONNEG>(v, c, q.lut, s_rec, q);
        store_samples<4>(reinterpret_cast<unsigned char *>(out + 4 * i), c, 2, 1);
    }
}


}  // namespace lh
