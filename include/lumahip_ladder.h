/* lumahip_ladder.h -- calls of liblumahip.so that score a rung of a delivery ladder against the archive's code planes.  The library
 * exports these symbols beside the other headers'; LUMAHIP_ABI_VERSION stays 5 (additions that change no existing symbol: detect them
 * with dlsym).  Including this header includes lumahip.h. */
#ifndef LUMAHIP_LADDER_H
#define LUMAHIP_LADDER_H

#include "lumahip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Half-resolution transcode distortion: how far GIVEN code planes of (w/2) x (h/2) -- the lower rung of a ladder as it came back from
 * the video decoder -- are from the planes lumahip_transcode_half_frames_device (include/lumahip_compare.h) would write for the
 * archive's source planes of w x h, in one launch: no scratch planes, no float frame, no second pass.
 *
 * What is compared (normative).  w and h are the SOURCE size, multiples of 4; the given set and every word belong to the target of
 * (w/2) x (h/2) luma samples in dst_profile's layout.  For every sample position of every target plane,
 *   e  is the unsigned sample lumahip_transcode_half_frames_device would store there for the same source planes, source quantizer,
 *      context quantizer, profiles and preScalings -- include/lumahip_compare.h has the normative text: the floats the decode
 *      stores, m = ((a + b) + (c + d)) * 0.25f in fp32 in that association, the target's encode of m --, masked to dst_profile's
 *      sample width (8-bit profiles keep the stored byte);
 *   g  is the unsigned sample present in the given plane, read as the decoder reads it (one byte, or two bytes little-endian; not
 *      clamped).
 *
 * lumahip_transcode_half_distortion_frames_device delivers per frame f and target plane p four uint64_t at
 *     out_dev[(f*3 + p)*4 + 0..3] = sse = sum (e-g)^2,   sad = sum |e-g|,   max_abs = max |e-g|,   n_differ = #{e != g}
 * over the plane's samples only -- the words and the layout of lumahip_transcode_distortion_frames_device.  out_dev (required, 8-byte
 * aligned, 12 * nframes words) is zero-initialised by the call.
 *
 * lumahip_transcode_half_distortion_map_frames_device delivers the same four words per plane for every block of `block` x `block`
 * luma pixels (block = 16, 32 or 64) OF THE HALF-SIZE TARGET, in the layout of lumahip_transcode_distortion_map_frames_device with
 * nbx = ceil((w/2) / block), nby = ceil((h/2) / block) (lumahip_distortion_map_dims(w/2, h/2, block, ...)):
 *     map_dev[(((f*nby + by)*nbx + bx)*3 + p)*4 + 0..3]
 * over the block's samples of the given planes: target luma pixels [bx*block, min(w/2, (bx+1)*block)) x [by*block, min(h/2,
 * (by+1)*block)), and on a 4:2:0 plane of dst_profile the samples co-sited with them.  The launch writes every one of the
 * nframes*nby*nbx*12 words exactly once, zeros included: map_dev needs no initialisation and none is queued.  Summing a frame's sse,
 * sad and n_differ over its blocks and taking the maximum of max_abs gives that frame's 12 words of the call above.
 *
 * All arithmetic behind the words is integer: they are bit-reproducible whatever the launch shape and order of arrival.  Both
 * plane sets are read only and may overlap each other; the words may share no byte with either.  The calls are asynchronous on the
 * context's stream, never wait on the host, take part in unordered sections and honour lumahip_tune "grid_enc", "lane_grid_enc",
 * "block" and "blocks_per_cu" (a workgroup is at most 512 threads, and at most 32 * block for the map).  The supported set is
 * lumahip_transcode_half_frames_device's, with the words in which a workgroup's waves meet (16, or 192 for the map) counted into its
 * on-chip memory beside both sides' tables.
 *
 * Errors come before anything is launched, and the words are then untouched: LUMAHIP_ERR_ARG for a block other than 16, 32 or 64,
 * null arguments, w or h not a multiple of 4, a bad profile, strides or frame strides that do not hold their planes (the source at
 * w x h, the given set at (w/2) x (h/2)), a null or misaligned output or one that shares a byte with either set, and in the host
 * form map_words < nbx*nby*12; LUMAHIP_ERR_STATE unless both quantizers are set; LUMAHIP_ERR_UNSUPPORTED outside the supported set.
 *
 * The host forms upload one frame's source planes and its given planes (no frame strides), run one launch, download the 12 words
 * into `out`, or the nbx*nby*12 words into `map`, and return synchronously.
 *
 * The parameter lists are those of lumahip_transcode_distortion_frames_device, lumahip_transcode_distortion_map_frames_device and
 * their host forms. */
int lumahip_transcode_half_distortion_frames_device(lumahip_ctx *ctx, const unsigned char *const src_planes_dev[3], const int src_stride[3],
                                                    const size_t src_plane_frame_stride[3], int src_profile, float src_sc, unsigned nframes,
                                                    unsigned w, unsigned h, const unsigned char *const given_planes_dev[3],
                                                    const int given_stride[3], const size_t given_plane_frame_stride[3], int dst_profile,
                                                    float dst_sc, uint64_t *out_dev);
int lumahip_transcode_half_distortion_map_frames_device(lumahip_ctx *ctx, const unsigned char *const src_planes_dev[3],
                                                        const int src_stride[3], const size_t src_plane_frame_stride[3], int src_profile,
                                                        float src_sc, unsigned nframes, unsigned w, unsigned h,
                                                        const unsigned char *const given_planes_dev[3], const int given_stride[3],
                                                        const size_t given_plane_frame_stride[3], int dst_profile, float dst_sc,
                                                        unsigned block, uint64_t *map_dev);
int lumahip_transcode_half_distortion_frame_host(lumahip_ctx *ctx, const unsigned char *const src_planes[3], const int src_stride[3],
                                                 int src_profile, float src_sc, unsigned w, unsigned h,
                                                 const unsigned char *const given_planes[3], const int given_stride[3], int dst_profile,
                                                 float dst_sc, uint64_t out[12]);
int lumahip_transcode_half_distortion_map_frame_host(lumahip_ctx *ctx, const unsigned char *const src_planes[3], const int src_stride[3],
                                                     int src_profile, float src_sc, unsigned w, unsigned h,
                                                     const unsigned char *const given_planes[3], const int given_stride[3],
                                                     int dst_profile, float dst_sc, unsigned block, uint64_t *map, size_t map_words);

#ifdef __cplusplus
}
#endif
#endif /* LUMAHIP_LADDER_H */
