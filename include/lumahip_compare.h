/* lumahip_compare.h -- calls of liblumahip.so that compare two sets of code planes as they are, and the header later additions to
 * the library go into: include/lumahip.h's and include/lumahip_measure.h's lists of declarations are closed, this one is open.  The
 * library exports these symbols beside the other headers'; LUMAHIP_ABI_VERSION stays 5 (additions that change no existing symbol:
 * detect them with dlsym).  Including this header includes lumahip.h. */
#ifndef LUMAHIP_COMPARE_H
#define LUMAHIP_COMPARE_H

#include "lumahip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Plane-to-plane measures: how far apart two sets of code planes are -- the planes a caller handed to a video encoder and the
 * planes the video decoder gave back, two decoded streams, or one stream against itself a frame later.
 *
 * Take two plane sets A and B of one profile (0..3), nframes frames of w x h, each set with its own base pointers, row strides
 * and frame strides.  Per sample position, e is the unsigned sample present in A and g the one in B.  Both are read as the decoder
 * reads them: one byte, or two bytes little-endian, not masked beyond that and not clamped to any table.
 *
 * Three results, with words, layouts, block membership, edge cuts and co-sited 4:2:0 chroma exactly as the existing calls define
 * them (lumahip_distortion_frames_device, lumahip_distortion_map_frames_device, lumahip_moments_map_frames_device):
 *   distortion      sse, sad, max_abs, n_differ per frame and plane:  out_dev[(f*3 + p)*4 + k], zero-initialised by the call;
 *   distortion map  the same four per block of 16, 32 or 64:          map_dev[(((f*nby + by)*nbx + bx)*3 + p)*4 + k], every word
 *                   written exactly once, no initialisation queued;
 *   moments map     sum e, sum g, sum e*e, sum g*g, sum e*g per block of 8, 16, 32 or 64:
 *                                                                     mom_dev[(((f*nby + by)*nbx + bx)*3 + p)*5 + k], likewise.
 * lumahip_distortion_map_dims and lumahip_moments_map_dims give the sizes.  All arithmetic is integer, so results are
 * bit-reproducible for every launch shape.
 *
 * No quantizer is needed.  The calls work on a context that never had lumahip_set_quantizer called (no LUMAHIP_ERR_STATE).  They
 * read neither quantizer and change neither.
 *
 * Overlap.  A and B may overlap each other in any way, since both are read only.  In particular B may be A one frame later
 * (b_planes_dev[p] = a_planes_dev[p] + a_plane_frame_stride[p], nframes - 1), which gives temporal differences from one buffer.
 * The output may share no byte with either set.
 *
 * Tuning and errors.  The calls are asynchronous on the context's stream and never wait on the host.  They take part in unordered
 * sections.  They honour lumahip_tune "grid_enc", "lane_grid_enc", "block" and "blocks_per_cu", as the other measuring calls do
 * (a workgroup of a map call is at most 32 * block threads, since it owns whole blocks).  Errors come before anything is
 * launched, and the output is then untouched: LUMAHIP_ERR_ARG for odd sizes, bad strides, a bad profile, a null plane pointer, or
 * a null or misaligned (8 bytes) output; LUMAHIP_ERR_ARG for an output overlapping either set, a block outside the call's set, or
 * host-form word counts that are too small.
 *
 * The host forms upload both plane sets of one frame (no frame strides), run one launch, download the 12 words into `out`, or
 * the nbx*nby*12 / nbx*nby*15 words into `map` / `mom`, and return synchronously. */
int lumahip_planes_distortion_frames_device(lumahip_ctx *ctx, const unsigned char *const a_planes_dev[3], const int a_stride[3],
                                            const size_t a_plane_frame_stride[3], unsigned nframes, unsigned w, unsigned h,
                                            const unsigned char *const b_planes_dev[3], const int b_stride[3],
                                            const size_t b_plane_frame_stride[3], int profile, uint64_t *out_dev);
int lumahip_planes_distortion_map_frames_device(lumahip_ctx *ctx, const unsigned char *const a_planes_dev[3], const int a_stride[3],
                                                const size_t a_plane_frame_stride[3], unsigned nframes, unsigned w, unsigned h,
                                                const unsigned char *const b_planes_dev[3], const int b_stride[3],
                                                const size_t b_plane_frame_stride[3], int profile, unsigned block, uint64_t *map_dev);
int lumahip_planes_moments_map_frames_device(lumahip_ctx *ctx, const unsigned char *const a_planes_dev[3], const int a_stride[3],
                                             const size_t a_plane_frame_stride[3], unsigned nframes, unsigned w, unsigned h,
                                             const unsigned char *const b_planes_dev[3], const int b_stride[3],
                                             const size_t b_plane_frame_stride[3], int profile, unsigned block, uint64_t *mom_dev);
int lumahip_planes_distortion_frame_host(lumahip_ctx *ctx, const unsigned char *const a_planes[3], const int a_stride[3], unsigned w,
                                         unsigned h, const unsigned char *const b_planes[3], const int b_stride[3], int profile,
                                         uint64_t out[12]);
int lumahip_planes_distortion_map_frame_host(lumahip_ctx *ctx, const unsigned char *const a_planes[3], const int a_stride[3], unsigned w,
                                             unsigned h, const unsigned char *const b_planes[3], const int b_stride[3], int profile,
                                             unsigned block, uint64_t *map, size_t map_words);
int lumahip_planes_moments_map_frame_host(lumahip_ctx *ctx, const unsigned char *const a_planes[3], const int a_stride[3], unsigned w,
                                          unsigned h, const unsigned char *const b_planes[3], const int b_stride[3], int profile,
                                          unsigned block, uint64_t *mom, size_t mom_words);

/* Content light level: what an HDR10 deliverable states about its own content -- how bright the brightest pixel is (MaxCLL) and how
 * bright the brightest frame is on average (MaxFALL), both over max(R, G, B) in cd/m2 -- as eight integers per frame, of frames as
 * they are or of a stream that is only held as code planes.
 *
 * The statistic (normative).  Inputs are a float frame F of w x h pixels and a `scale` that is finite and > 0; pass the stream's
 * preScaling to get cd/m2.  Per pixel, in fp32, nothing contracted:
 *   r = R * scale, g = G * scale, b = B * scale   one rounded multiply each (skipped when scale == 1.0f, since x * 1.0f is x);
 *   m = fmaxf(fmaxf(r, g), b)                     a NaN channel is ignored; m is NaN only if all three are;
 *   y = (0.212656f * r + 0.715158f * g) + 0.072186f * b
 *                                                 the Y row of the RGB -> XYZ matrix in its association order, not clamped; with
 *                                                 scale equal to the preScaling, the value whose clamp the Lu'v' encoder quantizes;
 *   q(v), in units of 1/256:  t = v * 256.0f;  q = 0 where !(t > 0) (NaN, negatives, both zeros, -inf);  q = 0xFFFFFFFF where
 *                             t >= 4294967296.0f (such pixels are counted as "over");  otherwise q = floor(t).
 * Per frame f, eight uint64_t words out[f * LUMAHIP_LIGHT_WORDS + k]:
 *   k  0  sum of q(m)      1  max of q(m)      2  pixels with m * 256 >= 2^32      3  pixels with m NaN
 *      4  sum of q(y)      5  max of q(y)      6  pixels with y * 256 >= 2^32      7  pixels with y NaN
 * All words are integers, so they are bit-reproducible for every launch shape and order of arrival (an 8K frame of saturated
 * pixels sums to 1.4e17, which fits).  MaxCLL = ceil(max over f of word 1 / 256), MaxFALL = ceil(max over f of word 0 /
 * (256 * w * h)), each capped at 65535 where it is stored in 16 bits: every pixel is in the divisor, as CTA-861.3 averages over the
 * whole picture.
 *
 * The plane-fed form is by definition the frame-fed form applied to the floats lumahip_decode_frames_device writes for those planes
 * under the context's quantizer and the given sc; no float frame is written.  It needs the quantizer (LUMAHIP_ERR_STATE without)
 * and the tables that call stages in on-chip memory: a transfer-function or chroma depth beyond 12 bits, or a YCbCr stream without
 * its y table, is LUMAHIP_ERR_UNSUPPORTED.  The frame-fed forms read no quantizer and work on a context that never had one.
 *
 * Frame layouts, strides counted in elements and alignment are the encode calls' (lumahip_encode_frames_device, _planar, _f16,
 * _planar_f16); the frames are only read, so their colour planes may overlap each other.  The calls are asynchronous on the
 * context's stream, never wait on the host, zero their words themselves, take part in unordered sections and honour lumahip_tune
 * "grid_enc", "lane_grid_enc", "block" and "blocks_per_cu".  Errors come before anything is launched, and the output is then
 * untouched: LUMAHIP_ERR_ARG for odd or zero sizes, nframes 0, a scale that is not finite and > 0, a null frame or plane pointer, bad
 * strides, a bad profile, a null or misaligned (8 bytes) out_dev, or an out_dev whose nframes * 64 bytes share a byte with what is read.
 *
 * The host forms upload one frame (packed floats, 3 * w * h) or one frame's planes, run one launch, download the eight words and
 * return synchronously. */
#define LUMAHIP_LIGHT_WORDS 8
int lumahip_light_level_frames_device(lumahip_ctx *ctx, const float *rgb_dev, size_t frame_stride, unsigned nframes, unsigned w, unsigned h,
                                      float scale, uint64_t *out_dev);
int lumahip_light_level_frames_device_planar(lumahip_ctx *ctx, const float *const planes_dev[3], size_t frame_stride, unsigned nframes,
                                             unsigned w, unsigned h, float scale, uint64_t *out_dev);
int lumahip_light_level_frames_device_f16(lumahip_ctx *ctx, const uint16_t *rgb_dev, size_t frame_stride, unsigned nframes, unsigned w,
                                          unsigned h, float scale, uint64_t *out_dev);
int lumahip_light_level_frames_device_planar_f16(lumahip_ctx *ctx, const uint16_t *const planes_dev[3], size_t frame_stride, unsigned nframes,
                                                 unsigned w, unsigned h, float scale, uint64_t *out_dev);
int lumahip_planes_light_level_frames_device(lumahip_ctx *ctx, const unsigned char *const planes_dev[3], const int stride[3],
                                             const size_t plane_frame_stride[3], unsigned nframes, unsigned w, unsigned h, int profile, float sc,
                                             float scale, uint64_t *out_dev);
int lumahip_light_level_frame_host(lumahip_ctx *ctx, const float *rgb, unsigned w, unsigned h, float scale, uint64_t out[8]);
int lumahip_planes_light_level_frame_host(lumahip_ctx *ctx, const unsigned char *const planes[3], const int stride[3], unsigned w, unsigned h,
                                          int profile, float sc, float scale, uint64_t out[8]);

/* Half-resolution transcode: the next rung of a delivery ladder straight from the archive's code planes -- source planes of w x h
 * under the context's source quantizer (lumahip_set_source_quantizer) to destination planes of (w/2) x (h/2) under its quantizer,
 * averaged 2x2 in linear light, in one launch and without a float frame (lumahip_transcode_frames_device is the full-size call).
 *
 * What is computed (normative).  w and h are the SOURCE size; the destination planes have (w/2) x (h/2) luma samples in
 * dst_profile's layout.  Per frame:
 *   d[c][y][x]   exactly the float lumahip_decode_frames_device would store for the source planes under the source quantizer,
 *                src_profile and src_sc (the division by src_sc carried out);
 *   m[c][Y][X] = ((d[c][2Y][2X] + d[c][2Y][2X+1]) + (d[c][2Y+1][2X] + d[c][2Y+1][2X+1])) * 0.25f
 *                in fp32, nothing contracted, in this association and no other (another order changes codes); a NaN's sign and
 *                payload reach no output;
 *   the destination planes are exactly what lumahip_encode_frames_device would write for m under the context's quantizer,
 *   dst_profile and dst_sc; stats_dev (nullable) is that call's {sum, min, max} of m's transformed channel 0 per frame -- for a
 *   YCbCr target the luminance, as the transcode call gives it.
 *
 * The device form is asynchronous on the context's stream, never waits on the host, takes part in unordered sections and honours
 * lumahip_tune "grid_enc", "lane_grid_enc", "block" and "blocks_per_cu", like the transcode call.  The host form uploads one
 * frame's source planes, runs one launch, downloads the destination planes and returns synchronously.  It has no mean_lum: the
 * reference has no half-resolution operation whose sequential sum such a mean could reproduce.
 *
 * Errors come before anything is launched, and the destination is then untouched: LUMAHIP_ERR_ARG for w or h not a multiple of 4
 * (the target must be even both ways), for strides or frame strides that do not hold their planes (the source at w x h, the
 * destination at (w/2) x (h/2)), for a source plane that shares a byte with a destination plane over the batch, for null
 * arguments and a bad profile; LUMAHIP_ERR_STATE unless both quantizers are set; LUMAHIP_ERR_UNSUPPORTED outside the transcode
 * call's supported set, unchanged: Lu'v' and YCbCr on either side in all 16 profile pairs, source tables of at most 12 bits,
 * a target with search mode 3 / 7 or the composite records, both sides' tables within 160 KiB of on-chip memory. */
int lumahip_transcode_half_frames_device(lumahip_ctx *ctx, const unsigned char *const src_planes_dev[3], const int src_stride[3],
                                         const size_t src_plane_frame_stride[3], int src_profile, float src_sc, unsigned nframes,
                                         unsigned w, unsigned h, unsigned char *const dst_planes_dev[3], const int dst_stride[3],
                                         const size_t dst_plane_frame_stride[3], int dst_profile, float dst_sc, float *stats_dev);
int lumahip_transcode_half_frame_host(lumahip_ctx *ctx, const unsigned char *const src_planes[3], const int src_stride[3], int src_profile,
                                      float src_sc, unsigned w, unsigned h, unsigned char *const dst_planes[3], const int dst_stride[3],
                                      int dst_profile, float dst_sc);

#ifdef __cplusplus
}
#endif
#endif /* LUMAHIP_COMPARE_H */
