#!/usr/bin/env python3
"""Generate tests/golden/ref_transcode.npz: code planes of one stream re-quantized into another stream's by the REFERENCE's own
code -- RefPlanes.decode (LumaDecoder::getVpxChannels + transformColorSpace(false)) followed by RefPlanes.encode
(transformColorSpace(true) + LumaEncoder::setChannels), i.e. what `lumadec | lumaenc` computes -- for the source planes that
ref_planes.npz already holds (`*_dec_plane*`: encoded frames with a few garbage codes, odd strides).

Needs oracle/_ref (the build container); the tests only read the result.  Stored: the target planes, their strides, the case list.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import oracle_py as o  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))

# name -> (ptf, bits, cs, bitsC, maxLum, minLum): the entries of make_golden.CONFIGS the cases use, and the one they add
CONFIGS = {
    "pq11_luv8": (o.PTF_PQ, 11, o.CS_LUV, 8, 1e4, 0.005),
    "pq10_ycbcr10": (o.PTF_PQ, 10, o.CS_YCBCR, 10, 1000.0, 0.01),
    "log12_luv8": (o.PTF_LOG, 12, o.CS_LUV, 8, 1e4, 0.005),
    "pq10_ycbcr10_4000": (o.PTF_PQ, 10, o.CS_YCBCR, 10, 4000.0, 0.01),
}
# case -> (source config, src_sc, target config, dst_sc); src_sc is the preScaling ref_planes.npz encoded the source with
CASES = {
    "luv_to_hdr10": ("pq11_luv8", 1.0, "pq10_ycbcr10", 20.0),
    "luv_to_log12": ("pq11_luv8", 1.0, "log12_luv8", 1.0),
    "hdr10_to_luv": ("pq10_ycbcr10", 20.0, "pq11_luv8", 1.0),
    "hdr10_to_hdr10_4000": ("pq10_ycbcr10", 20.0, "pq10_ycbcr10_4000", 20.0),
}
SIZES = ((34, 18), (64, 32))
SRC_PROFILES = (2, 3)
DST_PROFILE = 2


def key_of(case, w, h, src_profile):
    return "%s_%dx%d_p%d" % (case, w, h, src_profile)


def source_planes(pl, src, w, h, profile):
    """the `_dec_plane*` planes of ref_planes.npz and their strides"""
    k = "%s_%dx%d_p%d" % (src, w, h, profile)
    return [pl[k + "_dec_plane%d" % p] for p in range(3)], tuple(int(s) for s in pl[k + "_dec_stride"])


def transcode(decoder, encoder, planes, strides, w, h, src_sc, src_profile, dst_sc, dst_profile):
    """decode then encode, with anything that has .decode / .encode of the oracle's signature"""
    frame = decoder.decode(planes, strides, w, h, src_sc, src_profile)
    return encoder.encode(frame, dst_sc, dst_profile)[:2]


def main():
    o.build(ref=True)
    assert o.have_ref_planes()
    pl = np.load(os.path.join(OUT, "ref_planes.npz"))
    out = {}
    for case, (src, src_sc, dst, dst_sc) in CASES.items():
        dec, enc = o.RefPlanes(*CONFIGS[src]), o.RefPlanes(*CONFIGS[dst])
        for (w, h) in SIZES:
            for sp in SRC_PROFILES:
                planes, st = source_planes(pl, src, w, h, sp)
                tp, tst = transcode(dec, enc, planes, st, w, h, src_sc, sp, dst_sc, DST_PROFILE)
                k = key_of(case, w, h, sp)
                for p in range(3):
                    out[k + "_plane%d" % p] = tp[p]
                out[k + "_stride"] = np.array(tst, dtype=np.int32)
    out["cases"] = np.array(["%s: %s sc %g -> %s sc %g" % ((c,) + v) for c, v in CASES.items()])
    fn = os.path.join(OUT, "ref_transcode.npz")
    np.savez_compressed(fn, **out)
    print("ref_transcode.npz", os.path.getsize(fn), "bytes")


if __name__ == "__main__":
    main()
