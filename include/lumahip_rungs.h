/* lumahip_rungs.h -- calls of liblumahip.so that make the lower rungs of a delivery ladder from the archive's code planes, beyond the
 * half-size one of lumahip_compare.h.  The library exports these symbols beside the other headers'; LUMAHIP_ABI_VERSION stays 5
 * (additions that change no existing symbol: detect them with dlsym).  Including this header includes lumahip.h. */
#ifndef LUMAHIP_RUNGS_H
#define LUMAHIP_RUNGS_H

#include "lumahip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Quarter-resolution transcode: the third rung of a delivery ladder straight from the archive's code planes -- source planes of
 * w x h under the context's source quantizer (lumahip_set_source_quantizer) to destination planes of (w/4) x (h/4) under its
 * quantizer, averaged 4x4 in linear light, in one launch, without a float frame and without half-size planes
 * (lumahip_transcode_frames_device is the full-size call, lumahip_transcode_half_frames_device of lumahip_compare.h the half-size one).
 *
 * What is computed (normative).  w and h are the SOURCE size, multiples of 8; the destination planes have (w/4) x (h/4) luma samples
 * in dst_profile's layout.  Per frame, with d and m exactly as lumahip_compare.h defines them for the half-resolution call:
 *   d[c][y][x]   exactly the float lumahip_decode_frames_device would store for the source planes under the source quantizer,
 *                src_profile and src_sc (the division by src_sc carried out);
 *   m[c][y][x] = ((d[c][2y][2x] + d[c][2y][2x+1]) + (d[c][2y+1][2x] + d[c][2y+1][2x+1])) * 0.25f,   (w/2) x (h/2) floats;
 *   M[c][Y][X] = ((m[c][2Y][2X] + m[c][2Y][2X+1]) + (m[c][2Y+1][2X] + m[c][2Y+1][2X+1])) * 0.25f
 *                both in fp32, nothing contracted, in this association and no other (another order of the sixteen changes codes); a
 *                NaN's sign and payload reach no output;
 *   the destination planes are exactly what lumahip_encode_frames_device would write for M under the context's quantizer,
 *   dst_profile and dst_sc; stats_dev (nullable) is that call's {sum, min, max} of M's transformed channel 0 per frame -- for a
 *   YCbCr target the luminance, as the transcode call gives it.
 *
 * So the result is the half-resolution call's model applied twice TO FLOATS, with no quantization between the two averages.  It is
 * NOT what two half-resolution calls give: between those the half-size means are rounded to codes under some quantizer -- the
 * intermediate rung's -- and the second call averages the decoded codes, not the means; two roundings to codes replace one, and the
 * planes differ wherever the first rounding moves a mean far enough to move the final code.  (Two such calls also need the context's
 * source quantizer swapped between them.)
 *
 * The device form is asynchronous on the context's stream, never waits on the host, takes part in unordered sections and honours
 * lumahip_tune "grid_enc", "lane_grid_enc", "block" and "blocks_per_cu", like the transcode call.  The host form uploads one
 * frame's source planes, runs one launch, downloads the destination planes and returns synchronously.  It has no mean_lum: the
 * reference has no quarter-resolution operation whose sequential sum such a mean could reproduce.
 *
 * Errors come before anything is launched, and the destination is then untouched: LUMAHIP_ERR_ARG for w or h not a multiple of 8
 * (the target must be even both ways; "Invalid frame size WxH (quarter resolution: must be multiples of 8)"), for strides or frame
 * strides that do not hold their planes (the source at w x h, the destination at (w/4) x (h/4)), for a source plane that shares a
 * byte with a destination plane over the batch, for null arguments and a bad profile; LUMAHIP_ERR_STATE unless both quantizers are
 * set; LUMAHIP_ERR_UNSUPPORTED outside the transcode call's supported set, unchanged: Lu'v' and YCbCr on either side in all 16
 * profile pairs, source tables of at most 12 bits, a target with search mode 3 / 7 or the composite records, both sides' tables
 * within 160 KiB of on-chip memory.
 *
 * The parameter lists are those of lumahip_transcode_half_frames_device and lumahip_transcode_half_frame_host. */
int lumahip_transcode_quarter_frames_device(lumahip_ctx *ctx, const unsigned char *const src_planes_dev[3], const int src_stride[3],
                                            const size_t src_plane_frame_stride[3], int src_profile, float src_sc, unsigned nframes,
                                            unsigned w, unsigned h, unsigned char *const dst_planes_dev[3], const int dst_stride[3],
                                            const size_t dst_plane_frame_stride[3], int dst_profile, float dst_sc, float *stats_dev);
int lumahip_transcode_quarter_frame_host(lumahip_ctx *ctx, const unsigned char *const src_planes[3], const int src_stride[3],
                                         int src_profile, float src_sc, unsigned w, unsigned h, unsigned char *const dst_planes[3],
                                         const int dst_stride[3], int dst_profile, float dst_sc);

#ifdef __cplusplus
}
#endif
#endif /* LUMAHIP_RUNGS_H */
