// lumahip_pick.hpp -- which instantiation of the fused kernels (lh::k_encode / k_decode / k_transcode / k_distortion /
// k_distortion_map / k_moments_map / k_transcode_distortion / k_transcode_distortion_map / k_transcode_moments_map, luma_kernels.hpp)
// a launch takes (and of k_transcode_half and k_transcode_quarter).
// Naming a kernel here instantiates it, so this file decides which kernels exist, and the translation unit that instantiates
// a picker is the one that compiles its kernels: lumahip_encode.hip / lumahip_decode.hip take pick_enc<false> / pick_dec<false>
// (float frames), lumahip_encode_f16.hip / lumahip_decode_f16.hip take pick_enc<true> / pick_dec<true> (binary16 frames) and
// export them as pick_enc_f16 / pick_dec_f16; lumahip_transcode.hip takes pick_planes<TransFamily, 4 | 2>,
// lumahip_transcode_half.hip pick_planes<TransHalfFamily, 4 | 2>, lumahip_transcode_quarter.hip pick_planes<TransQuarterFamily, 4 | 2>.
// The eleven measuring
// units take one picker each and export it to the two dispatch functions (measure_planes_impl, measure_frames_impl):
// lumahip_transcode_distortion.hip pick_planes<TransDistFamily, 4 | 2> as pick_transdist; lumahip_transcode_distortion_map.hip
// pick_planes<TransDistMapFamily, 4 | 2> as pick_transdist_map; lumahip_transcode_moments_map.hip pick_planes<TransMomentsMapFamily,
// 4 | 2> as pick_transdist_moments_map; lumahip_transcode_half_distortion.hip pick_planes<TransHalfDistFamily, 4 | 2> as
// pick_transhalf_dist; lumahip_transcode_half_distortion_map.hip pick_planes<TransHalfDistMapFamily, 4 | 2> as pick_transhalf_dist_map;
// lumahip_distortion.hip / lumahip_distortion_f16.hip
// pick_dist<DistFamily, false / true> as pick_dist_f32 / _f16; lumahip_distortion_map.hip / lumahip_distortion_map_f16.hip
// pick_dist<DistMapFamily, false / true> as pick_dist_map_f32 / _f16; lumahip_moments_map.hip / lumahip_moments_map_f16.hip
// pick_dist<MomentsMapFamily, false / true> as pick_moments_map_f32 / _f16.  Included by those eighteen units only.
#pragma once
#include "lumahip_internal.hpp"

namespace lhost {

// mode: the search mode of the luminance table (lut_index.hpp LutMode), or for YCbCr 5 = the composite luma -> code records,
// 6 = the same + the half-input table.  vw == 4 or 2 for the record searches, 2 for the literal ones.
// IN16: no mode 5 (frames of halves take the table whenever it exists -- encode_frames_device_impl -- else the general kernel)
template <bool IN16, int CS, bool SUB>
static enc_kernel_t pick_enc_cs(int vw, int mode)
{
    using namespace lh;
    if constexpr (CS == CS_YCBCR) {
        if constexpr (!IN16)
            if (mode == 5)
                return vw == 4 ? k_encode<CS, SUB, 4, 5> : k_encode<CS, SUB, 2, 5>;
        if (mode == 6)
            return vw == 4 ? k_encode<CS, SUB, 4, 6, IN16> : k_encode<CS, SUB, 2, 6, IN16>;
    }
    if (mode == LUT_THRESH_LDS)
        return vw == 4 ? k_encode<CS, SUB, 4, 3, IN16> : k_encode<CS, SUB, 2, 3, IN16>;
    if (mode == LUT_THRESH_GLOBAL)
        return vw == 4 ? k_encode<CS, SUB, 4, 4, IN16> : k_encode<CS, SUB, 2, 4, IN16>;
    if (mode == LUT_LINKEY_LDS)
        return vw == 4 ? k_encode<CS, SUB, 4, 7, IN16> : k_encode<CS, SUB, 2, 7, IN16>;
    if (mode == LUT_LITERAL_LDS)
        return k_encode<CS, SUB, 2, 0, IN16>;
    if constexpr (IN16)
        if (mode != LUT_LITERAL_GLOBAL)
            return nullptr;
    return k_encode<CS, SUB, 2, 2, IN16>;
}

template <bool IN16>
static enc_kernel_t pick_enc(int cs, bool sub, int vw, int mode)
{
    using namespace lh;
    switch (cs) {
    case CS_LUV: return sub ? pick_enc_cs<IN16, CS_LUV, true>(vw, mode) : pick_enc_cs<IN16, CS_LUV, false>(vw, mode);
    case CS_RGB: return sub ? pick_enc_cs<IN16, CS_RGB, true>(vw, mode) : pick_enc_cs<IN16, CS_RGB, false>(vw, mode);
    case CS_YCBCR: return sub ? pick_enc_cs<IN16, CS_YCBCR, true>(vw, mode) : pick_enc_cs<IN16, CS_YCBCR, false>(vw, mode);
    case CS_XYZ: return sub ? pick_enc_cs<IN16, CS_XYZ, true>(vw, mode) : pick_enc_cs<IN16, CS_XYZ, false>(vw, mode);
    case CS_PACK:   // (frames that are already colour-transformed are floats)
        if constexpr (!IN16)
            return sub ? pick_enc_cs<IN16, CS_PACK, true>(vw, mode) : pick_enc_cs<IN16, CS_PACK, false>(vw, mode);
        break;
    }
    return nullptr;
}

// gl: the luminance table in global memory; disp: + the display epilogue; yt: the per-stream y table in LDS; rb: + red and
// blue from the per-stream tables in global memory.  OUT16: no display variants (binary16 stores only)
template <bool OUT16, int CS, bool SUB>
static dec_kernel_t pick_dec_cs(int vw, bool gl, bool disp, bool yt, bool rb)
{
    using namespace lh;
    if constexpr (CS == CS_YCBCR) {
        if (yt && rb && !gl && !disp)
            return vw == 4 ? k_decode<CS, SUB, 4, false, false, true, true, OUT16> : k_decode<CS, SUB, 2, false, false, true, true, OUT16>;
        if (yt && !gl && !disp)
            return vw == 4 ? k_decode<CS, SUB, 4, false, false, true, false, OUT16> : k_decode<CS, SUB, 2, false, false, true, false, OUT16>;
    }
    if (disp) {
        if constexpr (OUT16)
            return nullptr;
        else if (gl)
            return k_decode<CS, SUB, 2, true, true>;
        else
            return vw == 4 ? k_decode<CS, SUB, 4, false, true> : k_decode<CS, SUB, 2, false, true>;
    }
    if (gl)
        return k_decode<CS, SUB, 2, true, false, false, false, OUT16>;
    return vw == 4 ? k_decode<CS, SUB, 4, false, false, false, false, OUT16> : k_decode<CS, SUB, 2, false, false, false, false, OUT16>;
}

template <bool OUT16>
static dec_kernel_t pick_dec(int cs, bool sub, int vw, bool gl, bool disp, bool yt, bool rb)
{
    using namespace lh;
    switch (cs) {
    case CS_LUV: return sub ? pick_dec_cs<OUT16, CS_LUV, true>(vw, gl, disp, yt, rb) : pick_dec_cs<OUT16, CS_LUV, false>(vw, gl, disp, yt, rb);
    case CS_RGB: return sub ? pick_dec_cs<OUT16, CS_RGB, true>(vw, gl, disp, yt, rb) : pick_dec_cs<OUT16, CS_RGB, false>(vw, gl, disp, yt, rb);
    case CS_YCBCR: return sub ? pick_dec_cs<OUT16, CS_YCBCR, true>(vw, gl, disp, yt, rb) : pick_dec_cs<OUT16, CS_YCBCR, false>(vw, gl, disp, yt, rb);
    case CS_XYZ: return sub ? pick_dec_cs<OUT16, CS_XYZ, true>(vw, gl, disp, yt, rb) : pick_dec_cs<OUT16, CS_XYZ, false>(vw, gl, disp, yt, rb);
    case CS_PACK:   // (the unpack-only decode writes dequantized floats; no _f16 entry point runs it)
        if constexpr (!OUT16)
            return sub ? pick_dec_cs<OUT16, CS_PACK, true>(vw, gl, disp, yt, rb) : pick_dec_cs<OUT16, CS_PACK, false>(vw, gl, disp, yt, rb);
        break;
    }
    return nullptr;
}

// The plane-fed kernels: lh::k_transcode (TransFamily, named by lumahip_transcode.hip only), lh::k_transcode_distortion
// (TransDistFamily, named by lumahip_transcode_distortion.hip only), lh::k_transcode_distortion_map (TransDistMapFamily, named by
// lumahip_transcode_distortion_map.hip only) and lh::k_transcode_moments_map (TransMomentsMapFamily, named by
// lumahip_transcode_moments_map.hip only), the same keys kernel for kernel.  A family says what its kernels
// are and how many threads per workgroup they are compiled for (transcode_plan clamps the launch to it).
struct TransFamily {
    using kernel_t = trans_kernel_t;
    template <int CSD, bool SUBD, int CSE, bool SUBE, int VW, int LM>
    static kernel_t kernel() { return lh::k_transcode<CSD, SUBD, CSE, SUBE, VW, LM>; }
    static int bound(bool) { return 1024; }
};
struct TransHalfFamily {   // lh::k_transcode_half, named by lumahip_transcode_half.hip only (launch bound: lh::transhalf_threads_bound, which transcode_plan clamps the launch to)
    using kernel_t = trans_kernel_t;
    template <int CSD, bool SUBD, int CSE, bool SUBE, int VW, int LM>
    static kernel_t kernel() { return lh::k_transcode_half<CSD, SUBD, CSE, SUBE, VW, LM>; }
};
struct TransQuarterFamily {   // lh::k_transcode_quarter, named by lumahip_transcode_quarter.hip only (launch bound: lh::transquarter_threads_bound, which transcode_plan clamps the launch to)
    using kernel_t = trans_kernel_t;
    template <int CSD, bool SUBD, int CSE, bool SUBE, int VW, int LM>
    static kernel_t kernel() { return lh::k_transcode_quarter<CSD, SUBD, CSE, SUBE, VW, LM>; }
};
struct TransDistFamily {
    using kernel_t = transdist_kernel_t;
    template <int CSD, bool SUBD, int CSE, bool SUBE, int VW, int LM>
    static kernel_t kernel() { return lh::k_transcode_distortion<CSD, SUBD, CSE, SUBE, VW, LM>; }
    static int bound(bool any_y) { return any_y ? lh::TransDistBound<lh::CS_YCBCR, lh::CS_YCBCR>::value : lh::TransDistBound<lh::CS_LUV, lh::CS_LUV>::value; }
};

struct TransDistMapFamily {   // (launch bound: TransDistFamily's, which transcode_plan clamps every measuring launch to)
    using kernel_t = transdist_map_kernel_t;
    template <int CSD, bool SUBD, int CSE, bool SUBE, int VW, int LM>
    static kernel_t kernel() { return lh::k_transcode_distortion_map<CSD, SUBD, CSE, SUBE, VW, LM>; }
};
struct TransMomentsMapFamily {   // (launch bound: lh::transmoments_threads_bound, which transcode_plan clamps the launch to)
    using kernel_t = transdist_map_kernel_t;
    template <int CSD, bool SUBD, int CSE, bool SUBE, int VW, int LM>
    static kernel_t kernel() { return lh::k_transcode_moments_map<CSD, SUBD, CSE, SUBE, VW, LM>; }
};
// lh::k_transcode_half_distortion / lh::k_transcode_half_distortion_map, named by lumahip_transcode_half_distortion.hip /
// lumahip_transcode_half_distortion_map.hip only (launch bounds: lh::transhalfdist_threads_bound / lh::transhalfmap_threads_bound, which
// transcode_plan clamps the launch to).  The source families lh::transhalfdist_vw4 denies have no VW 4 kernel: the plan gives them VW 2
struct TransHalfDistFamily {
    using kernel_t = transdist_kernel_t;
    template <int CSD, bool SUBD, int CSE, bool SUBE, int VW, int LM>
    static kernel_t kernel()
    {
        if constexpr (VW == 4 && !lh::transhalfdist_vw4(CSD, SUBD, CSE))
            return nullptr;
        else
            return lh::k_transcode_half_distortion<CSD, SUBD, CSE, SUBE, VW, LM>;
    }
};
struct TransHalfDistMapFamily {
    using kernel_t = transdist_map_kernel_t;
    template <int CSD, bool SUBD, int CSE, bool SUBE, int VW, int LM>
    static kernel_t kernel()
    {
        if constexpr (VW == 4 && !lh::transhalfdist_vw4(CSD, SUBD, CSE))
            return nullptr;
        else
            return lh::k_transcode_half_distortion_map<CSD, SUBD, CSE, SUBE, VW, LM>;
    }
};

// source colour space / subsampling, target colour space / subsampling, the target's search mode -- Lu'v': LUT_THRESH_LDS or
// LUT_LINKEY_LDS, YCbCr: 5 = the composite records.  nullptr: outside the supported set.
// VW a template parameter so that, like the pickers above, only the unit that names it compiles the kernels
template <typename F, int VW, int CSD, bool SUBD>
static typename F::kernel_t pick_planes_src(int cse, bool sube, int mode)
{
    using namespace lh;
    if (cse == CS_LUV && mode == LUT_THRESH_LDS)
        return sube ? F::template kernel<CSD, SUBD, CS_LUV, true, VW, 3>() : F::template kernel<CSD, SUBD, CS_LUV, false, VW, 3>();
    if (cse == CS_LUV && mode == LUT_LINKEY_LDS)
        return sube ? F::template kernel<CSD, SUBD, CS_LUV, true, VW, 7>() : F::template kernel<CSD, SUBD, CS_LUV, false, VW, 7>();
    if (cse == CS_YCBCR && mode == 5)
        return sube ? F::template kernel<CSD, SUBD, CS_YCBCR, true, VW, 5>() : F::template kernel<CSD, SUBD, CS_YCBCR, false, VW, 5>();
    return nullptr;
}

template <typename F, int VW>
static typename F::kernel_t pick_planes(int csd, bool subd, int cse, bool sube, int mode)
{
    using namespace lh;
    switch (csd) {
    case CS_LUV: return subd ? pick_planes_src<F, VW, CS_LUV, true>(cse, sube, mode) : pick_planes_src<F, VW, CS_LUV, false>(cse, sube, mode);
    case CS_YCBCR: return subd ? pick_planes_src<F, VW, CS_YCBCR, true>(cse, sube, mode) : pick_planes_src<F, VW, CS_YCBCR, false>(cse, sube, mode);
    }
    return nullptr;
}

// The frame-fed measuring kernels: lh::k_distortion (DistFamily, named by lumahip_distortion.hip / lumahip_distortion_f16.hip only) and
// lh::k_distortion_map (DistMapFamily, named by lumahip_distortion_map.hip / lumahip_distortion_map_f16.hip only) and lh::k_moments_map
// (MomentsMapFamily, named by lumahip_moments_map.hip / lumahip_moments_map_f16.hip only), the same keys kernel for kernel.
struct DistFamily {
    using kernel_t = dist_kernel_t;
    template <int CS, bool SUB, int VW, int LM, bool IN16>
    static kernel_t kernel() { return lh::k_distortion<CS, SUB, VW, LM, IN16>; }
};
struct DistMapFamily {
    using kernel_t = map_kernel_t;
    template <int CS, bool SUB, int VW, int LM, bool IN16>
    static kernel_t kernel() { return lh::k_distortion_map<CS, SUB, VW, LM, IN16>; }
};
struct MomentsMapFamily {   // (launch bound: lh::moments_threads_bound, which distortion_plan clamps the launch to)
    using kernel_t = map_kernel_t;
    template <int CS, bool SUB, int VW, int LM, bool IN16>
    static kernel_t kernel() { return lh::k_moments_map<CS, SUB, VW, LM, IN16>; }
};

// Search records in LDS only.  mode: LUT_THRESH_LDS or LUT_LINKEY_LDS, or for YCbCr 5 = the composite records (float frames),
// 6 = the same + the half-input table (binary16 frames).  nullptr: outside that set.
template <typename F, bool IN16, int CS, bool SUB>
static typename F::kernel_t pick_dist_cs(int vw, int mode)
{
    using namespace lh;
    if constexpr (CS == CS_YCBCR) {
        if constexpr (!IN16) {
            if (mode == 5)
                return vw == 4 ? F::template kernel<CS, SUB, 4, 5, false>() : F::template kernel<CS, SUB, 2, 5, false>();
        } else {
            if (mode == 6)
                return vw == 4 ? F::template kernel<CS, SUB, 4, 6, true>() : F::template kernel<CS, SUB, 2, 6, true>();
        }
    }
    if (mode == LUT_THRESH_LDS)
        return vw == 4 ? F::template kernel<CS, SUB, 4, 3, IN16>() : F::template kernel<CS, SUB, 2, 3, IN16>();
    if (mode == LUT_LINKEY_LDS)
        return vw == 4 ? F::template kernel<CS, SUB, 4, 7, IN16>() : F::template kernel<CS, SUB, 2, 7, IN16>();
    return nullptr;
}

template <typename F, bool IN16>
static typename F::kernel_t pick_dist(int cs, bool sub, int vw, int mode)
{
    using namespace lh;
    switch (cs) {
    case CS_LUV: return sub ? pick_dist_cs<F, IN16, CS_LUV, true>(vw, mode) : pick_dist_cs<F, IN16, CS_LUV, false>(vw, mode);
    case CS_RGB: return sub ? pick_dist_cs<F, IN16, CS_RGB, true>(vw, mode) : pick_dist_cs<F, IN16, CS_RGB, false>(vw, mode);
    case CS_YCBCR: return sub ? pick_dist_cs<F, IN16, CS_YCBCR, true>(vw, mode) : pick_dist_cs<F, IN16, CS_YCBCR, false>(vw, mode);
    case CS_XYZ: return sub ? pick_dist_cs<F, IN16, CS_XYZ, true>(vw, mode) : pick_dist_cs<F, IN16, CS_XYZ, false>(vw, mode);
    }
    return nullptr;
}

}  // namespace lhost
