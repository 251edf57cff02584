/* lumahip_measure.h -- measuring calls of liblumahip.so added after include/lumahip.h's list of declarations was closed.  The
 * library exports them beside that header's symbols; LUMAHIP_ABI_VERSION stays 5 (additions that change no existing symbol:
 * detect them with dlsym).  Including this header includes lumahip.h. */
#ifndef LUMAHIP_MEASURE_H
#define LUMAHIP_MEASURE_H

#include "lumahip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Transcode moments map: the five sums of the moments map (lumahip_moments_map_frames_device), per plane, for every block of
 * `block` x `block` luma pixels (block = 8, 16, 32 or 64) of the target, with e taken from the transcode of SOURCE code planes
 * instead of the encode of float frames -- what a structural-similarity index in the code domain needs in a pipeline that holds
 * code planes and never float frames.  One launch, no float frames, no scratch planes; e and g are exactly the transcode distortion
 * calls': e is the unsigned sample lumahip_transcode_frames_device would store for the same source planes, source quantizer,
 * context quantizer, profiles and preScalings, masked to dst_profile's sample width, and g the unsigned sample present in the
 * given plane, read as the decoder reads it.  Layout and block membership are exactly the moments map's: with
 * nbx = ceil(w / block), nby = ceil(h / block) (lumahip_moments_map_dims serves both moments maps) the words of frame f, block
 * (bx, by), plane p are
 *     mom_dev[(((f*nby + by)*nbx + bx)*3 + p)*5 + 0..4] = sum e, sum g, sum e*e, sum g*g, sum e*g
 * over the block's samples of the GIVEN planes: luma pixels [bx*block, min(w, (bx+1)*block)) x [by*block, min(h, (by+1)*block)), and
 * on a 4:2:0 plane of dst_profile the samples co-sited with them (the source's subsampling plays no part): 120 bytes per block.
 * The launch writes every one of the nframes*nby*nbx*15 words exactly once: mom_dev needs no initialisation and none is queued.
 * All arithmetic is integer: the map is the same from run to run whatever the launch shape; sum e*e - 2 sum e*g + sum g*g is the
 * transcode distortion map's sse of the same block (summed over a frame's blocks: lumahip_transcode_distortion_frames_device's),
 * and adding the words of 2 x 2 neighbouring blocks gives the map of twice the block size -- which is also how a caller forms
 * overlapping windows (16 x 16 windows at stride 8 from 8-blocks); the calls themselves deliver disjoint blocks only.
 * Arguments, supported set, stream, unordered sections and the honoured lumahip_tune keys are those of
 * lumahip_transcode_distortion_map_frames_device ("block": a workgroup is at most 32 * block threads for this call, since it owns
 * whole blocks -- 256 for blocks of 8 --, and at most the 512 threads its kernels are compiled for: 1024 only for Lu'v' -> Lu'v'
 * with planes that allow no more than two pixels per thread and row), with mom_dev (required, 8-byte aligned, its
 * nframes*nby*nbx*120 bytes sharing no byte with either plane set; the two plane sets may overlap each other) in the place of
 * map_dev, and the 480 words in which a workgroup's waves meet counted into its LDS beside both sides' tables.  Never waits on the
 * host.  Errors, all before anything is launched (mom_dev is then untouched): those of that call, and LUMAHIP_ERR_ARG for a block
 * other than 8, 16, 32 or 64 and, in the host form, for mom_words < nbx*nby*15.
 * The host form uploads both plane sets of one frame, runs one launch, downloads the nbx*nby*15 words into `mom` and returns
 * synchronously. */
int lumahip_transcode_moments_map_frames_device(lumahip_ctx *ctx, const unsigned char *const src_planes_dev[3], const int src_stride[3],
                                                const size_t src_plane_frame_stride[3], int src_profile, float src_sc, unsigned nframes,
                                                unsigned w, unsigned h, const unsigned char *const given_planes_dev[3],
                                                const int given_stride[3], const size_t given_plane_frame_stride[3], int dst_profile,
                                                float dst_sc, unsigned block, uint64_t *mom_dev);
int lumahip_transcode_moments_map_frame_host(lumahip_ctx *ctx, const unsigned char *const src_planes[3], const int src_stride[3],
                                             int src_profile, float src_sc, unsigned w, unsigned h,
                                             const unsigned char *const given_planes[3], const int given_stride[3], int dst_profile,
                                             float dst_sc, unsigned block, uint64_t *mom, size_t mom_words);

#ifdef __cplusplus
}
#endif
#endif /* LUMAHIP_MEASURE_H */
