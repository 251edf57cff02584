"""What the moments map's tests share: the numpy model the kernels are held to (built on tests/support/host.py plane_samples), the
folds that tie a map to the map of twice the block size and to the distortion map, and the wrapper of the device call.  torch is
imported inside the functions, so that importing this module needs no GPU.

Helpers here assert with an explicit message: pytest rewrites `assert` in test modules only."""
import numpy as np

from tests.support.host import GUARD, OUT_FILL, plane_samples

MOM_BLOCKS = (8, 16, 32, 64)
MOM_SYMBOLS = ["lumahip_moments_map_dims", "lumahip_moments_map_frames_device", "lumahip_moments_map_frames_device_planar",
               "lumahip_moments_map_frames_device_f16", "lumahip_moments_map_frames_device_planar_f16", "lumahip_moments_map_frame_host"]


def _block_sums(a, b, nby, nbx):
    """(nby, nbx) sums of a (rows, columns) int64 array over b x b blocks cut at the array's edges"""
    rows, cols = a.shape
    assert (nby - 1) * b < rows and (nbx - 1) * b < cols, ("a block without samples", a.shape, b, nby, nbx)
    pad = np.zeros((nby * b, nbx * b), dtype=np.int64)
    pad[:rows, :cols] = a
    return pad.reshape(nby, b, nbx, b).sum(axis=(1, 3))


def expected_moments_map(planes_e, planes_g, w, h, profile, block):
    """(nby, nbx, 3, 5) uint64: per block of block x block luma pixels -- on a 4:2:0 chroma plane the block/2 x block/2 samples
    co-sited with them -- cut at the frame's edges, and per plane {sum e, sum g, sum e^2, sum g^2, sum e g} of two sets of three
    (rows, stride) uint8 planes"""
    nbx, nby = -(-w // block), -(-h // block)
    out = np.zeros((nby, nbx, 3, 5), dtype=np.uint64)
    for p in range(3):
        b = block // 2 if (p and profile in (0, 2)) else block
        e, g = plane_samples(planes_e[p], w, h, profile, p), plane_samples(planes_g[p], w, h, profile, p)
        for k, a in enumerate((e, g, e * e, g * g, e * g)):
            out[:, :, p, k] = _block_sums(a, b, nby, nbx).astype(np.uint64)
    return out


def expect_moments(enc, ebufs, given, gbufs, block):
    """expected_moments_map of every frame of two plane sets (anything with .frame(bufs, f), .nf, .w, .h, .profile)"""
    return np.stack([expected_moments_map(enc.frame(ebufs, f), given.frame(gbufs, f), enc.w, enc.h, enc.profile, block)
                     for f in range(enc.nf)])


def fold_2x2(m):
    """the map of twice the block size from a (..., nby, nbx, 3, 5) map: the words of 2 x 2 neighbouring blocks added, an odd last row
    or column alone"""
    nby, nbx = m.shape[-4:-2]
    pad = np.zeros(m.shape[:-4] + (2 * -(-nby // 2), 2 * -(-nbx // 2), 3, 5), dtype=np.uint64)
    pad[..., :nby, :nbx, :, :] = m
    return pad[..., 0::2, 0::2, :, :] + pad[..., 1::2, 0::2, :, :] + pad[..., 0::2, 1::2, :, :] + pad[..., 1::2, 1::2, :, :]


def sse_of(m):
    """(..., 3) uint64: sum e^2 - 2 sum e g + sum g^2 of a (..., 3, 5) moments map -- the distortion map's sse"""
    s = m.astype(np.int64)
    d = s[..., 2] - 2 * s[..., 4] + s[..., 3]
    assert (d >= 0).all(), "a negative sum of squares"
    return d.astype(np.uint64)


def mom_nwords(nf, w, h, block):
    return nf * (-(-w // block)) * (-(-h // block)) * 15


def mom_words(buf, nf, w, h, block):
    """the moments map of a call as (nf, nby, nbx, 3, 5) uint64, after checking the guard words behind it; buf: the mom_nwords + GUARD
    int64 of tests/support/device.py map_buf, or a numpy array of them"""
    a = buf.cpu().numpy() if hasattr(buf, "cpu") else np.asarray(buf)
    assert np.all(a[-GUARD:] == OUT_FILL), "guard words behind the moments map"
    return a[:-GUARD].view(np.uint64).reshape(nf, -(-h // block), -(-w // block), 3, 5)


def mom_map(c, fr, sc, given, block, form="packed"):
    """the map of lumahip_moments_map_frames_device in one of its four forms"""
    import torch

    from tests.support.device import _frame_fed, map_buf
    buf = map_buf(mom_nwords(fr.nf, fr.w, fr.h, block))
    _frame_fed(c, "moments_map_frames_device", fr, form,
               (fr.fs, fr.nf, fr.w, fr.h, sc, given.profile, given.ptrs, given.st, given.pfs, block, buf.data_ptr()))
    torch.cuda.synchronize()
    return mom_words(buf, fr.nf, fr.w, fr.h, block)
