"""What the transcode moments map's tests share: the symbols, the wrapper of the device call and the properties the GPU test's inputs
must have for a wrong kernel not to pass.  The numpy model, the folds and the buffers are tests/support/moments.py's, host.py's and
device.py's.  torch is imported inside the functions, so that importing this module needs no GPU.

Helpers here assert with an explicit message: pytest rewrites `assert` in test modules only."""
import re

import numpy as np

from tests.support.host import BLOCKS, MAP_SIZES, map_perturbed, perturb, plane_samples
from tests.support.moments import MOM_BLOCKS, mom_nwords, mom_words

TMOM_SYMBOLS = ["lumahip_transcode_moments_map_frames_device", "lumahip_transcode_moments_map_frame_host"]
TMOM_HEADER = "lumahip_measure.h"
ALL_BLOCKS_AT = ((264, 70), (34, 18))


def blocks_at(w, h, it):
    """the blocks the pairs test runs at size (w, h) in its it-th case: all four at ALL_BLOCKS_AT, one -- rotating -- elsewhere"""
    return MOM_BLOCKS if (w, h) in ALL_BLOCKS_AT else (MOM_BLOCKS[it % 4],)


def kept_block(w, h, blocks):
    """the block whose rightmost column and bottom row frame 1 of a case's given planes keeps as written, one set of given planes serving
    every block of the case: the largest with more than one block column and row -- its kept samples are whole blocks of every smaller
    size, and the larger ones have one column or row, where nothing is asked -- or, without one, the largest"""
    many = [b for b in blocks if -(-w // b) > 1 and -(-h // b) > 1]
    return max(many) if many else max(blocks)


def pairs_cases():
    """(it, source profile, target profile, w, h) of the pairs test, in its order: all 16 profile pairs x MAP_SIZES"""
    out, it = [], 0
    for sp in range(4):
        for dp in range(4):
            for (w, h) in MAP_SIZES:
                it += 1
                out.append((it, sp, dp, w, h))
    return out


class HostPlanes:
    """nf frames of three (rows, stride) planes in host memory, with what map_perturbed / expect_moments ask of a plane set"""

    def __init__(self, frames, w, h, profile):
        self.frames, self.nf, self.w, self.h, self.profile = frames, len(frames), w, h, profile

    def frame(self, bufs, f):
        return bufs[f]


def given_frames(rng, enc, ebufs, w, h, profile, block):
    """The given planes of the GPU test for the planes a call wrote: map_perturbed -- every frame perturbed densely, frame 1 keeping its
    rightmost block column and bottom block row as written -- with two amendments that make Seg != See hold in every plane of every
    frame.  Where the map has one block column or row, map_perturbed's frame 1 is the written frame itself: it is perturbed like the
    others instead.  And a plane whose perturbation cancels in sum e (g - e) gets one more difference, at its largest sample outside
    the kept column and row."""
    frames = map_perturbed(rng, enc, ebufs, w, h, profile, block)
    nbx, nby = -(-w // block), -(-h // block)
    bps = 2 if profile > 1 else 1
    for f in range(enc.nf):
        orig = enc.frame(ebufs, f)
        if f == 1 and (nbx == 1 or nby == 1):
            frames[f] = perturb(rng, orig, w, h, profile, frac=0.5)
        for p in range(3):
            e, g = plane_samples(orig[p], w, h, profile, p), plane_samples(frames[f][p], w, h, profile, p)
            if int((e * (g - e)).sum()) != 0:
                continue
            b = block // 2 if (p and profile in (0, 2)) else block
            free = e if (nbx == 1 or nby == 1) else e[:(nby - 1) * b, :(nbx - 1) * b]
            y, x = np.unravel_index(int(np.argmax(free)), free.shape)
            if free[y, x] == 0:   # (a plane of zeros: Seg == See == 0 whatever is given)
                continue
            top = 0xFFFF if bps == 2 else 0xFF
            v = next(v for v in (int(e[y, x]) - 1, int(e[y, x]) - 2, int(e[y, x]) + 1) if 0 <= v <= top and v != int(g[y, x]))
            frames[f][p][y, x * bps] = v & 0xFF
            if bps == 2:
                frames[f][p][y, x * bps + 1] = v >> 8
    return frames


def declarations(header_text):
    """{name: [parameter texts]} of every `int lumahip_x(...);` of a header without function-pointer parameters"""
    hdr = re.sub(r"/\*.*?\*/", " ", header_text, flags=re.S)
    hdr = re.sub(r"//[^\n]*|^[ \t]*#[^\n]*", " ", hdr, flags=re.M)
    return {m.group(1): [t.strip() for t in " ".join(m.group(2).split()).split(",")]
            for m in re.finditer(r"\bint\s+(lumahip_\w+)\s*\(([^()]*)\)\s*;", hdr)}


def tmom(c, src, src_sc, given, dst_sc, block, src_ptrs=None):
    """the map of lumahip_transcode_moments_map_frames_device"""
    import torch

    from tests.support.device import map_buf
    buf = map_buf(mom_nwords(src.nf, src.w, src.h, block))
    c.transcode_moments_map_frames_device(src.ptrs if src_ptrs is None else src_ptrs, src.st, src.pfs, src.profile, src_sc, src.nf, src.w,
                                          src.h, given.ptrs, given.st, given.pfs, given.profile, dst_sc, block, buf.data_ptr())
    torch.cuda.synchronize()
    return mom_words(buf, src.nf, src.w, src.h, block)


def own_planes_moments(m):
    """whether a (..., 3, 5) moments map is one of planes against themselves: Se == Sg and See == Sgg == Seg, and not all zeros"""
    return bool(m.any() and np.array_equal(m[..., 0], m[..., 1]) and np.array_equal(m[..., 2], m[..., 3]) and
                np.array_equal(m[..., 2], m[..., 4]))


def inputs_cannot_pass_a_wrong_kernel(exp, tag):
    """asserted on the numpy expectation (nf, nby, nbx, 3, 5) of perturbed planes: in every plane of every frame the cross moment is not
    the second moment (a kernel that read e for g, or g for e, fails); with more than one block column and row, every plane has a block
    without a difference and at least half of its blocks have one"""
    s = exp.astype(np.int64)
    frame = s.sum(axis=(1, 2))                                    # (nf, 3, 5)
    assert (frame[..., 4] != frame[..., 2]).all(), tag + ("a plane with Seg == See",)
    differ = (s[..., 2] - 2 * s[..., 4] + s[..., 3]) != 0         # (nf, nby, nbx, 3)
    if differ.shape[1] > 1 and differ.shape[2] > 1:
        for p in range(3):
            assert (~differ[..., p]).any(), tag + (p, "no block without a difference")
            assert 2 * np.count_nonzero(differ[..., p]) >= differ[..., p].size, tag + (p, "fewer than half the blocks differ")


def frame_sse(m):
    """(nf, 3) uint64: See - 2 Seg + Sgg summed over the blocks of every frame of a (nf, nby, nbx, 3, 5) map"""
    s = m.astype(np.int64).sum(axis=(1, 2))
    return (s[..., 2] - 2 * s[..., 4] + s[..., 3]).astype(np.uint64)


__all__ = ["ALL_BLOCKS_AT", "BLOCKS", "MOM_BLOCKS", "TMOM_HEADER", "TMOM_SYMBOLS", "HostPlanes", "blocks_at", "declarations", "frame_sse",
           "given_frames", "inputs_cannot_pass_a_wrong_kernel", "kept_block", "own_planes_moments", "pairs_cases", "tmom"]
