"""What the plane-to-plane measures' tests share (include/lumahip_compare.h): the symbols, the cases, the builder of the two plane sets
the GPU test compares, the properties those inputs must have for a wrong kernel not to pass, and one wrapper per device call.  The numpy
models, the folds and the buffers are tests/support/host.py's, moments.py's, transcode_moments.py's and device.py's.  torch is imported
inside the functions, so that importing this module needs no GPU.

Helpers here assert with an explicit message: pytest rewrites `assert` in test modules only."""
import numpy as np

from tests.support.host import BLOCKS, GUARD, OUT_FILL, expect, expect_map, fold_map, nwords, plane_rows, random_frames
from tests.support.moments import MOM_BLOCKS, expect_moments, mom_nwords, mom_words
from tests.support.transcode_moments import HostPlanes, given_frames, inputs_cannot_pass_a_wrong_kernel, kept_block

PM_HEADER = "lumahip_compare.h"
PM_DEVICE = ["lumahip_planes_distortion_frames_device", "lumahip_planes_distortion_map_frames_device",
             "lumahip_planes_moments_map_frames_device"]
PM_HOST = ["lumahip_planes_distortion_frame_host", "lumahip_planes_distortion_map_frame_host", "lumahip_planes_moments_map_frame_host"]
PM_SYMBOLS = PM_DEVICE + PM_HOST
PM_METHODS = ["planes_distortion_frames_device", "planes_distortion_map_frames_device", "planes_moments_map_frames_device",
              "planes_distortion_frame", "planes_distortion_map_frame", "planes_moments_map_frame"]
# four pixels and two pixels per thread, several block rows and columns, ragged edges both ways, all in one workgroup's tile
PM_SIZES = [(6, 4), (34, 18), (258, 6), (260, 6), (264, 70), (64, 32)]
NF = 3


def numpy_cases():
    """(profile, w, h) of the GPU test against numpy, in its order"""
    return [(profile, w, h) for profile in range(4) for (w, h) in PM_SIZES]


def case_rng(profile, w, h):
    return np.random.default_rng(1000 * w + 10 * h + profile)


def two_sets(rng, w, h, profile, nf=NF, pad=5):
    """The two plane sets of a case, as lists of nf frames of three (rows, stride) uint8 planes with rows `pad` bytes longer than their
    samples: A random bytes (codes no table has included), B the transcode moments test's given_frames of A -- every frame
    perturbed densely, frame 1 keeping the rightmost block column and the bottom block row of the largest block with more than one
    column and row, Seg != See in every plane."""
    st = tuple(plane_rows(w, h, profile, p)[1] + pad for p in range(3))
    a = random_frames(rng, w, h, profile, nf, st)
    b = given_frames(rng, HostPlanes(a, w, h, profile), a, w, h, profile, kept_block(w, h, MOM_BLOCKS))
    return a, b, st


def model(a, b, w, h, profile):
    """numpy's words of two lists of frames: (per-frame (nf, 3, 4), {block: (nf, nby, nbx, 3, 4)}, {block: (nf, nby, nbx, 3, 5)})"""
    ha, hb = HostPlanes(a, w, h, profile), HostPlanes(b, w, h, profile)
    return (expect(ha, a, hb, b), {blk: expect_map(ha, a, hb, b, blk) for blk in BLOCKS},
            {blk: expect_moments(ha, a, hb, b, blk) for blk in MOM_BLOCKS})


def folds(frame, maps, moms, tag):
    """a call's results agree among themselves: every distortion map folds to the per-frame words, the moments give the map's sse, and
    2 x 2 moment blocks add up to the next block size"""
    from tests.support.moments import fold_2x2, sse_of
    for blk, m in maps.items():
        assert np.array_equal(np.stack([fold_map(m[f]) for f in range(m.shape[0])]), frame), tag + (blk, "the map folds to the frame's words")
        assert np.array_equal(sse_of(moms[blk]), m[..., 0]), tag + (blk, "See - 2 Seg + Sgg is the map's sse")
    for blk in MOM_BLOCKS[:-1]:
        assert np.array_equal(fold_2x2(moms[blk]), moms[2 * blk]), tag + (blk, "2 x 2 moment blocks")


def inputs_cannot_pass(frame, maps, moms, tag):
    """asserted on numpy's words of a case of two_sets: every plane of every frame differs between A and B; Seg != See in every plane;
    wherever a map has more than one row and column it has a block without a difference and at least half of its blocks have one; no
    map is all zeros"""
    assert (frame[..., 3] > 0).all(), tag + ("a plane without a difference",)
    for blk, m in moms.items():
        inputs_cannot_pass_a_wrong_kernel(m, tag + (blk,))
        assert m.any(), tag + (blk, "a moments map of zeros")
    for blk, m in maps.items():
        assert m.any(), tag + (blk, "a distortion map of zeros")
        nd = m[..., 3]
        if nd.shape[1] > 1 and nd.shape[2] > 1:
            for p in range(3):
                assert (nd[..., p] == 0).any(), tag + (blk, p, "no block without a difference")
                assert 2 * np.count_nonzero(nd[..., p]) >= nd[..., p].size, tag + (blk, p, "fewer than half the blocks differ")


def swapped(m):
    """a (..., 3, 5) moments map with A and B exchanged: words 0 <-> 1 and 2 <-> 3, the cross moment as it is"""
    return m[..., [1, 0, 3, 2, 4]]


# ---- the device calls: a, b are tests/support/device.py Planes; *_ptrs / nf override a set's base pointers and the frame count
def _args(a, b, a_ptrs, b_ptrs, nf):
    return (a.ptrs if a_ptrs is None else a_ptrs, a.st, a.pfs, a.nf if nf is None else nf, a.w, a.h,
            b.ptrs if b_ptrs is None else b_ptrs, b.st, b.pfs, a.profile)


def frame_buf(nf):
    """what out_dev holds before a call: nf * 12 words of the 0xC3 pattern and GUARD more behind them, which the call must leave alone
    (its memset and its atomics at out[frame * 12 + .] included)"""
    import torch

    from tests.support.device import dev
    return torch.full((nf * 12 + GUARD,), OUT_FILL, dtype=torch.int64, device=dev())


def frame_words(buf, nf):
    """the words of a per-frame call as (nf, 3, 4) uint64, after checking the guard words behind them"""
    a = buf.cpu().numpy() if hasattr(buf, "cpu") else np.asarray(buf)
    assert a.size == nf * 12 + GUARD and np.all(a[-GUARD:] == OUT_FILL), "guard words behind the per-frame words"
    return a[:-GUARD].view(np.uint64).reshape(nf, 3, 4)


def pdist(c, a, b, a_ptrs=None, b_ptrs=None, nf=None):
    """the twelve words per frame of lumahip_planes_distortion_frames_device"""
    import torch
    n = a.nf if nf is None else nf
    o = frame_buf(n)
    c.planes_distortion_frames_device(*_args(a, b, a_ptrs, b_ptrs, nf), o.data_ptr())
    torch.cuda.synchronize()
    return frame_words(o, n)


def pmap(c, a, b, block, a_ptrs=None, b_ptrs=None, nf=None):
    """the map of lumahip_planes_distortion_map_frames_device"""
    import torch

    from tests.support.device import map_buf
    from tests.support.host import map_words
    n = a.nf if nf is None else nf
    buf = map_buf(nwords(n, a.w, a.h, block))
    c.planes_distortion_map_frames_device(*_args(a, b, a_ptrs, b_ptrs, nf), block, buf.data_ptr())
    torch.cuda.synchronize()
    return map_words(buf, n, a.w, a.h, block)


def pmom(c, a, b, block, a_ptrs=None, b_ptrs=None, nf=None):
    """the map of lumahip_planes_moments_map_frames_device"""
    import torch

    from tests.support.device import map_buf
    n = a.nf if nf is None else nf
    buf = map_buf(mom_nwords(n, a.w, a.h, block))
    c.planes_moments_map_frames_device(*_args(a, b, a_ptrs, b_ptrs, nf), block, buf.data_ptr())
    torch.cuda.synchronize()
    return mom_words(buf, n, a.w, a.h, block)


def all_three(c, a, b, **kw):
    """(per-frame words, {block: distortion map}, {block: moments map}) of the three calls, all blocks"""
    return pdist(c, a, b, **kw), {blk: pmap(c, a, b, blk, **kw) for blk in BLOCKS}, {blk: pmom(c, a, b, blk, **kw) for blk in MOM_BLOCKS}


def same_results(got, want, tag):
    """two (frame, maps, moms) triples, word for word"""
    assert np.array_equal(got[0], want[0]), tag + ("per-frame words", got[0], want[0])
    for blk in want[1]:
        assert np.array_equal(got[1][blk], want[1][blk]), tag + ("distortion map", blk)
    for blk in want[2]:
        assert np.array_equal(got[2][blk], want[2][blk]), tag + ("moments map", blk)
