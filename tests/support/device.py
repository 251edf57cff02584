"""What the GPU tests share: the `L` fixture, contexts on torch's stream, frames and code planes in device buffers, and one wrapper per
device call.  torch is imported inside the functions, so that importing this module needs no GPU."""
import os

import numpy as np
import pytest

from tests.support.host import (GAP, GUARD, OUT_FILL, SENTINEL, blank_planes, frames_buffer, gaps_intact, layout, map_words, nwords,
                                planes_from_frames, random_frames, same_bits)
from tests.support.tools import ROOT


@pytest.fixture(scope="module")
def L():
    import lumahdrv_amd
    return lumahdrv_amd


def dev():
    import torch
    return torch.device("cuda:0")


def ctx(L, cfg, src_cfg=None, literal=False, quantizer=True):
    """a context on torch's current stream, so that its launches are ordered with the tensors' fills and copies: quantizer = cfg,
    source quantizer = src_cfg"""
    import torch
    c = L.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    if literal:
        c.tune("force_literal", 1)
    if quantizer:
        c.set_quantizer(*cfg, L.build_lut(cfg[0], cfg[1], cfg[4], cfg[5]))
    if src_cfg is not None:
        c.set_source_quantizer(*src_cfg, L.build_lut(src_cfg[0], src_cfg[1], src_cfg[4], src_cfg[5]))
    return c


def table_for(o, cfg):
    if cfg[0] in (o.PTF_PSI, o.PTF_JND_HDRVDP):
        d = os.path.join(ROOT, "lumahdrv_amd", "data")
        nm = "psi" if cfg[0] == o.PTF_PSI else "jnd_hdrvdp"
        return np.fromfile(os.path.join(d, "ptf_%s_%d.f32" % (nm, cfg[1])), dtype="<f4")
    return None


def pair(L, o, cfg):
    """(HIP quantizer, oracle) for a configuration tuple (ptf, bits, cs, bitsC, maxLum, minLum)"""
    q = L.LumaQuantizer()
    q.setQuantizer(*cfg)
    orc = o.Oracle(*cfg, table=table_for(o, cfg))
    assert same_bits(q.getMapping(), orc.mapping), "the quantizer's table is not the oracle's"
    return q, orc


class Frames:
    """frames on the device, frame f at base + f * fs elements; the gap between frames holds sentinel bytes, and so do the `base`
    elements in front of the first frame (base 2 puts float frames 8 bytes off a 16-byte boundary)"""

    def __init__(self, frames, dtype=np.float32, pad=4, base=0):
        import torch
        nf, _, h, w = frames.shape
        self.nf, self.w, self.h, self.n = nf, w, h, w * h
        self.fs = 3 * self.n + pad
        self.host = frames_buffer(frames, dtype, pad)
        self.front = base * np.dtype(dtype).itemsize
        self.bytes = np.concatenate([np.full(self.front, SENTINEL, dtype=np.uint8), self.host.view(np.uint8).ravel()])
        self.t = torch.from_numpy(self.bytes.copy()).to(dev())

    @property
    def ptr(self):
        return self.t.data_ptr() + self.front

    def unchanged(self):
        return np.array_equal(self.t.cpu().numpy(), self.bytes)


class FloatOut:
    """the buffer a decode call writes nf frames of floats (or halves) into: frame f at base + f * fs elements, fs = 3 w h + pad; the
    sentinel everywhere before the call"""

    def __init__(self, nf, w, h, dtype=np.float32, pad=4, base=0):
        import torch
        self.nf, self.w, self.h, self.n3, self.dtype = nf, w, h, 3 * w * h, np.dtype(dtype)
        self.fs = self.n3 + pad
        self.front = base * self.dtype.itemsize
        self.t = torch.full((self.front + nf * self.fs * self.dtype.itemsize,), SENTINEL, dtype=torch.uint8, device=dev())

    @property
    def ptr(self):
        return self.t.data_ptr() + self.front

    def frames(self):
        """(nf, 3, h, w) of dtype, after checking the bytes in front of the first frame and behind every frame"""
        a = self.t.cpu().numpy()
        assert np.all(a[:self.front] == SENTINEL), "bytes in front of the first frame"
        fr = a[self.front:].reshape(self.nf, self.fs * self.dtype.itemsize)
        assert np.all(fr[:, self.n3 * self.dtype.itemsize:] == SENTINEL), "bytes behind a frame"
        return np.ascontiguousarray(fr[:, :self.n3 * self.dtype.itemsize]).view(self.dtype).reshape(self.nf, 3, self.h, self.w)

    def untouched(self):
        return bool((self.t == SENTINEL).all())


def _strides(L, w, h, profile, strides):
    """the given row strides, or the library's own for this size"""
    return tuple(int(s) for s in strides) if strides is not None else L.plane_geometry(w, h, profile)[2]


class Planes:
    """nf frames of code planes on the device: plane p of frame f at buf[p] + base + f * pfs[p], rows st[p] bytes apart; `fill` is what
    the buffers were given (the sentinel everywhere by default).  `base` bytes of sentinel lie in front of every plane (torch's
    buffers are aligned far beyond 16 bytes, so base is the planes' misalignment); `gap`: one number or one per plane"""

    def __init__(self, L, w, h, profile, nf, fill=None, strides=None, gap=GAP, base=0):
        import torch
        self.w, self.h, self.profile, self.nf, self.gap, self.base = w, h, profile, nf, gap, base
        self.st = _strides(L, w, h, profile, strides)
        self.hs, self.size, self.pfs = layout(w, h, profile, self.st, gap)
        if fill is None:
            fill = blank_planes(w, h, profile, nf, self.st, gap, base)
        self.fill = [np.ascontiguousarray(f) for f in fill]
        self.t = [torch.from_numpy(self.fill[p]).to(dev()) for p in range(3)]

    @property
    def ptrs(self):
        return [t.data_ptr() + self.base for t in self.t]

    def host(self):
        return [t.cpu().numpy() for t in self.t]

    def frame(self, bufs, f):
        """frame f as three (rows, stride) arrays"""
        return [bufs[p][self.base + f * self.pfs[p]: self.base + f * self.pfs[p] + self.size[p]].reshape(self.hs[p], self.st[p])
                for p in range(3)]

    def unchanged(self):
        return all(np.array_equal(a, b) for a, b in zip(self.host(), self.fill))

    def gaps_intact(self, bufs):
        return gaps_intact(bufs, self.w, self.h, self.profile, self.nf, self.st, self.gap, self.base)


def from_frames(L, frames, w, h, profile, strides=None, *, padding):
    """Planes holding the given frames (lists of three (rows, >= row bytes) arrays), the sentinel in every gap; behind each row's
    samples the sentinel (padding="sentinel") or what the source rows hold there (padding="source")"""
    fill = planes_from_frames(frames, w, h, profile, _strides(L, w, h, profile, strides), padding)
    return Planes(L, w, h, profile, len(frames), fill=fill, strides=strides)


def on_device(L, hp):
    """the Planes of a host plane set (tests/support/measuring.py HostPlanes): the same bytes in the same layout"""
    return Planes(L, hp.w, hp.h, hp.profile, hp.nf, fill=hp.bufs, strides=hp.st, gap=hp.gap, base=hp.base)


def random_planes(L, rng, w, h, profile, nf, strides=None):
    """random bytes in the samples (out-of-range codes included), the sentinel in every row padding and gap"""
    frames = random_frames(rng, w, h, profile, nf, _strides(L, w, h, profile, strides))
    return from_frames(L, frames, w, h, profile, strides=strides, padding="source")


# ---- output buffers
def out_buf(nf):
    import torch
    return torch.full((nf * 12,), OUT_FILL, dtype=torch.int64, device=dev())


def out_words(out, nf):
    return out.cpu().numpy().view(np.uint64).reshape(nf, 3, 4)


def map_buf(nwords):
    import torch
    return torch.full((nwords + GUARD,), OUT_FILL, dtype=torch.int64, device=dev())


# ---- the device calls
def stats_buf(nf):
    """the 3 nf floats a call writes its per-frame {sum, min, max} into, NaN before the call"""
    import torch
    return torch.full((3 * nf,), float("nan"), dtype=torch.float32, device=dev())


def encode(c, L, fr, sc, profile, strides=None, stats=False):
    """the planes lumahip_encode_frames_device writes for these frames, as host buffers + their Planes; stats: + the (nf, 3)
    {sum, min, max} it reports"""
    import torch
    pl = Planes(L, fr.w, fr.h, profile, fr.nf, strides=strides)
    sd = stats_buf(fr.nf) if stats else None
    c.encode_frames_device(fr.ptr, fr.fs, fr.nf, fr.w, fr.h, sc, profile, pl.ptrs, pl.st, pl.pfs, sd.data_ptr() if stats else None)
    torch.cuda.synchronize()
    return (pl, pl.host(), sd.cpu().numpy().reshape(fr.nf, 3)) if stats else (pl, pl.host())


def _frame_fed(c, call, fr, form, args):
    """one of the four forms of a frame-fed measuring call: packed / planar floats, packed / planar halves"""
    esz = fr.t.element_size() * fr.host.dtype.itemsize
    planar = [fr.ptr + k * fr.n * esz for k in range(3)]
    suffix = {"packed": "", "planar": "_planar", "f16": "_f16", "planar_f16": "_planar_f16"}[form]
    getattr(c, call + suffix)(planar if form.startswith("planar") else fr.ptr, *args)


def dist(c, fr, sc, given, form="packed"):
    """the twelve words per frame of lumahip_distortion_frames_device in one of its four forms"""
    import torch
    o = out_buf(fr.nf)
    _frame_fed(c, "distortion_frames_device", fr, form,
               (fr.fs, fr.nf, fr.w, fr.h, sc, given.profile, given.ptrs, given.st, given.pfs, o.data_ptr()))
    torch.cuda.synchronize()
    return out_words(o, fr.nf)


def dist_map(c, fr, sc, given, block, form="packed"):
    """the map of lumahip_distortion_map_frames_device in one of its four forms"""
    import torch
    buf = map_buf(nwords(fr.nf, fr.w, fr.h, block))
    _frame_fed(c, "distortion_map_frames_device", fr, form,
               (fr.fs, fr.nf, fr.w, fr.h, sc, given.profile, given.ptrs, given.st, given.pfs, block, buf.data_ptr()))
    torch.cuda.synchronize()
    return map_words(buf, fr.nf, fr.w, fr.h, block)


def fused(c, src, src_sc, dst, dst_sc, stats=None):
    c.transcode_frames_device(src.ptrs, src.st, src.pfs, src.profile, src_sc, src.nf, src.w, src.h,
                              dst.ptrs, dst.st, dst.pfs, dst.profile, dst_sc, stats.data_ptr() if stats is not None else None)


def two_calls(cd, ce, src, src_sc, dst, dst_sc, stats=None):
    """decode under cd's quantizer into a float buffer, encode it under ce's"""
    import torch
    n3 = 3 * src.w * src.h
    buf = torch.empty(src.nf * n3, dtype=torch.float32, device=dev())
    cd.decode_frames_device(src.ptrs, src.st, src.pfs, src.nf, src.w, src.h, src.profile, src_sc, buf.data_ptr(), n3)
    ce.encode_frames_device(buf.data_ptr(), n3, src.nf, src.w, src.h, dst_sc, dst.profile, dst.ptrs, dst.st, dst.pfs,
                            stats.data_ptr() if stats is not None else None)
    return buf


def transcoded(c, L, src, src_sc, dp, dst_sc, strides=None, gap=GAP, base=0, stats=False):
    """what lumahip_transcode_frames_device writes for src into sentinel-filled planes (rows `strides` apart, `gap` bytes behind a
    frame, `base` bytes into their buffers): its Planes and their host buffers; stats: + the (nf, 3) {sum, min, max} it reports"""
    import torch
    dst = Planes(L, src.w, src.h, dp, src.nf, strides=strides, gap=gap, base=base)
    sd = stats_buf(src.nf) if stats else None
    fused(c, src, src_sc, dst, dst_sc, sd)
    torch.cuda.synchronize()
    return (dst, dst.host(), sd.cpu().numpy().reshape(src.nf, 3)) if stats else (dst, dst.host())


def measure(c, src, src_sc, given, dst_sc, out=None):
    """the twelve words per frame of lumahip_transcode_distortion_frames_device"""
    import torch
    o = out_buf(src.nf) if out is None else out
    c.transcode_distortion_frames_device(src.ptrs, src.st, src.pfs, src.profile, src_sc, src.nf, src.w, src.h,
                                         given.ptrs, given.st, given.pfs, given.profile, dst_sc, o.data_ptr())
    torch.cuda.synchronize()
    return out_words(o, src.nf)


def tmap(c, src, src_sc, given, dst_sc, block, src_ptrs=None):
    """the map of lumahip_transcode_distortion_map_frames_device"""
    import torch
    buf = map_buf(nwords(src.nf, src.w, src.h, block))
    c.transcode_distortion_map_frames_device(src.ptrs if src_ptrs is None else src_ptrs, src.st, src.pfs, src.profile, src_sc, src.nf, src.w,
                                             src.h, given.ptrs, given.st, given.pfs, given.profile, dst_sc, block, buf.data_ptr())
    torch.cuda.synchronize()
    return map_words(buf, src.nf, src.w, src.h, block)


def inputs_as_before(src, sbefore, given, gbefore, tag, sentinels=True):
    """both plane sets byte for byte what they were, and (planes built here, not the fixture's rows) the sentinel in every padding and gap"""
    for a, b in zip(sbefore + gbefore, src.host() + given.host()):
        assert np.array_equal(a, b), tag + ("an input plane changed",)
    if sentinels:
        assert src.gaps_intact(sbefore) and given.gaps_intact(gbefore), tag
