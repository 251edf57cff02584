"""What the content light level tests share (include/lumahip_compare.h): the symbols, the numpy model of the statistic -- float32
operations, np.fmax, the three cases of q written out, uint64 sums --, a scalar Python restatement of it, the builder of the frames the GPU
test measures, the properties those frames must have for a wrong kernel not to pass, the output buffers and one wrapper per device call.
torch is imported inside the functions, so that importing this module needs no GPU.

Helpers here assert with an explicit message: pytest rewrites `assert` in test modules only."""
import math
import struct

import numpy as np

from tests.support.host import GUARD, OUT_FILL

LL_HEADER = "lumahip_compare.h"
LL_DEVICE = ["lumahip_light_level_frames_device", "lumahip_light_level_frames_device_planar", "lumahip_light_level_frames_device_f16",
             "lumahip_light_level_frames_device_planar_f16", "lumahip_planes_light_level_frames_device"]
LL_HOST = ["lumahip_light_level_frame_host", "lumahip_planes_light_level_frame_host"]
LL_SYMBOLS = LL_DEVICE + LL_HOST
LL_METHODS = ["light_level_frames_device", "light_level_frames_device_planar", "light_level_frames_device_f16",
              "light_level_frames_device_planar_f16", "planes_light_level_frames_device", "light_level_frame", "planes_light_level_frame"]
WORDS = 8
# one tile, two pixels per thread, two only with a ragged last tile, four, four with several tiles both ways, four in one tile
LL_SIZES = [(6, 4), (34, 18), (258, 6), (260, 6), (264, 70), (64, 32)]
SCALES = (1.0, 20.0, 0.01)
NF = 3
OVER = 0xFFFFFFFF
F32 = np.float32
KR, KG, KB = F32(0.212656), F32(0.715158), F32(0.072186)
JUST_OVER = F32(16777216.0)                       # * 256 == 2^32
JUST_UNDER = np.nextafter(JUST_OVER, F32(0))      # the float below it
PEAKS = (None, F32(4000.0), F32(9000.0))          # the corner pixel of frames 1 and 2 (frame 0: +inf); binary16 values


# ---- the model
def _q(v):
    """q of a float32 array: (uint64 values, over mask)"""
    with np.errstate(over="ignore", invalid="ignore"):
        t = v * F32(256.0)
    assert t.dtype == np.float32
    over = t >= F32(4294967296.0)
    mid = (t > 0) & ~over
    q = np.zeros(t.shape, dtype=np.uint64)
    q[mid] = np.floor(t[mid]).astype(np.uint64)
    q[over] = OVER
    return q, over


def pixel_values(frame, scale):
    """(m, y) of a (3, h, w) float32 frame, float32 arithmetic in the statistic's order"""
    f = np.asarray(frame)
    assert f.dtype == np.float32 and f.shape[0] == 3
    r, g, b = f[0], f[1], f[2]
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        if F32(scale) != F32(1.0):
            r, g, b = r * F32(scale), g * F32(scale), b * F32(scale)
        m = np.fmax(np.fmax(r, g), b)
        y = (KR * r + KG * g) + KB * b
    assert m.dtype == np.float32 and y.dtype == np.float32
    return m, y


def model(frame, scale):
    """the eight words of one (3, h, w) float32 frame"""
    out = np.zeros(WORDS, dtype=np.uint64)
    for k, v in enumerate(pixel_values(frame, scale)):
        q, over = _q(v)
        out[4 * k:4 * k + 4] = (q.sum(dtype=np.uint64), q.max(), np.count_nonzero(over), np.count_nonzero(np.isnan(v)))
    return out


def model_frames(frames, scale):
    """(nf, 8) uint64"""
    return np.stack([model(f, scale) for f in frames])


def _f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def scalar_model(frame, scale):
    """the same words pixel by pixel in Python: every operation rounded to float32 through struct, fmaxf and the three cases written out"""
    _, h, w = frame.shape
    scale = _f32(scale)
    words = [0] * WORDS
    for yy in range(h):
        for xx in range(w):
            r, g, b = (float(frame[c, yy, xx]) for c in range(3))
            if scale != 1.0:
                r, g, b = _f32(r * scale), _f32(g * scale), _f32(b * scale)

            def fmaxf(p, q):
                return q if math.isnan(p) else p if math.isnan(q) else max(p, q)
            m = fmaxf(fmaxf(r, g), b)
            lum = _f32(_f32(_f32(float(KR) * r) + _f32(float(KG) * g)) + _f32(float(KB) * b))
            for k, v in enumerate((m, lum)):
                t = _f32(v * 256.0) if not math.isinf(v) else v
                if not t > 0:
                    q = 0
                elif t >= 4294967296.0:
                    q = OVER
                    words[4 * k + 2] += 1
                else:
                    q = int(math.floor(t))
                words[4 * k + 0] += q
                words[4 * k + 1] = max(words[4 * k + 1], q)
                words[4 * k + 3] += math.isnan(v)
    return np.array(words, dtype=np.uint64)


# ---- the frames
def planted():
    """[(row, column, (R, G, B))] of frame 0: one channel NaN, all three NaN, -inf, negatives, -0, a denormal, just over, just under,
    a pixel whose luminance is over too; all inside 6 x 4 and none in the last row or column"""
    nan, inf = F32(np.nan), F32(np.inf)
    return [(0, 0, (nan, F32(5), F32(7))), (0, 1, (nan, nan, nan)), (0, 2, (-inf, F32(1), F32(2))), (0, 3, (F32(-3), F32(-1), F32(-2))),
            (0, 4, (F32(-0.0), F32(-0.0), F32(-0.0))), (1, 0, (F32(1e-40), F32(0), F32(0))), (1, 1, (JUST_OVER, F32(1), F32(1))),
            (1, 2, (JUST_UNDER, F32(1), F32(1))), (1, 3, (F32(2e7), F32(2e7), F32(2e7)))]


def frames(w, h, halves=False):
    """NF distinct (3, h, w) float32 frames, log-uniform over 1e-3 .. 1e2 and brighter from frame to frame.  The brightest pixel of
    frame f is its bottom right corner -- in the last row AND the last column -- and sits in channel f % 3: +inf in frame 0, PEAKS[f]
    after it.  Frame 0 also holds planted(); frames 1 and 2 hold no NaN and nothing over.  halves: narrowed to binary16 and widened
    again (just over becomes inf, the denormal zero), the values both the float and the binary16 calls are then given"""
    out = []
    for f in range(NF):
        rng = np.random.default_rng(w * 977 + h * 31 + f)
        a = (np.exp(rng.uniform(np.log(1e-3), np.log(1e2), size=(3, h, w))) * (1 + f)).astype(np.float32)
        a[:, h - 1, w - 1] = F32(1)
        a[f % 3, h - 1, w - 1] = F32(np.inf) if f == 0 else PEAKS[f]
        if f == 0:
            for (yy, xx, rgb) in planted():
                a[:, yy, xx] = rgb
        out.append(a)
    out = np.stack(out)
    if halves:
        from tests.support.host import widen_halves
        with np.errstate(over="ignore"):
            out = widen_halves(out.astype(np.float16))
    return out


def dropped(fr, what):
    """the frames with a channel (0, 1, 2) zeroed, or without their last row / last column"""
    a = np.array(fr, copy=True)
    if what in (0, 1, 2):
        a[:, what] = 0
        return a
    return np.ascontiguousarray(a[:, :, :-1, :] if what == "row" else a[:, :, :, :-1])


def inputs_cannot_pass(fr, scale, tag):
    """asserted on the model's words of frames(): see tests/test_light_level_host.py"""
    words = model_frames(fr, scale)
    nf, _, h, w = fr.shape
    m = [pixel_values(f, scale)[0] for f in fr]
    for f in range(nf):
        # the brightest pixel: the corner, in channel f % 3, alone there
        with np.errstate(invalid="ignore"):
            top = np.nanmax(m[f])
            where = np.argwhere(m[f] == top)
        assert (h - 1, w - 1) in [tuple(p) for p in where], tag + (f, "the maximum is not in the corner")
        assert all(p[0] == h - 1 or p[1] == w - 1 for p in where) or f == 0, tag + (f, "a maximum outside the last row and column")
        sc = fr[f][:, h - 1, w - 1] * F32(scale)
        assert int(np.argmax(sc)) == f % 3 and np.count_nonzero(sc == sc.max()) == 1, tag + (f, "the corner's channel")
    for k in (0, 1, 4, 5):
        assert len(set(int(x) for x in words[:, k])) == nf, tag + (k, "a word is the same in two frames", words[:, k])
    for k in (2, 3, 6, 7):
        assert words[0, k] > 0 and words[1, k] == 0 and words[2, k] == 0, tag + (k, "counts", words[:, k])
    # what a kernel that drops something would report
    for what in (0, 1, 2, "row", "column"):
        other = model_frames(dropped(fr, what), scale)
        assert np.all(other[:, 0] != words[:, 0]), tag + (what, "word 0 survives the drop", other[:, 0], words[:, 0])
        # word 1: in every frame without a pixel over (frame 0 stays saturated by its planted pixels); a channel: in its own frame
        frames_hit = [f for f in (1, 2) if what in ("row", "column") or f % 3 == what]
        assert all(other[f, 1] != words[f, 1] for f in frames_hit), tag + (what, "word 1 survives the drop")
        if what in ("row", "column", 0):
            assert other[0, 2] < words[0, 2], tag + (what, "frame 0's corner is counted as over")
    if F32(scale) != F32(1):
        plain = model_frames(fr, 1.0)
        assert np.all(plain[:, 0] != words[:, 0]) and np.all(plain[1:, 1] != words[1:, 1]), tag + ("the scale changes nothing",)
    return words


# ---- buffers and device calls
def light_buf(nf):
    """what out_dev holds before a call: nf * 8 words of the 0xC3 pattern and GUARD more behind them, which the call must leave alone
    (its memset and its atomics at out[frame * 8 + .] included)"""
    import torch

    from tests.support.device import dev
    return torch.full((nf * WORDS + GUARD,), OUT_FILL, dtype=torch.int64, device=dev())


def light_words(buf, nf):
    """the words of a call as (nf, 8) uint64, after checking the guard words behind them"""
    a = buf.cpu().numpy()
    assert a.size == nf * WORDS + GUARD and np.all(a[-GUARD:] == OUT_FILL), "guard words behind the light-level words"
    return a[:-GUARD].view(np.uint64).reshape(nf, WORDS)


def light(c, fr, scale, form="packed"):
    """the eight words per frame of lumahip_light_level_frames_device in one of its four forms; fr: tests/support/device.py Frames
    (of halves for the two _f16 forms) or FloatOut -- packed frames at fr.ptr, fr.fs elements apart"""
    import torch
    esz = 2 if form.endswith("f16") else 4
    planar = [fr.ptr + k * fr.w * fr.h * esz for k in range(3)]
    suffix = {"packed": "", "planar": "_planar", "f16": "_f16", "planar_f16": "_planar_f16"}[form]
    o = light_buf(fr.nf)
    getattr(c, "light_level_frames_device" + suffix)(planar if form.startswith("planar") else fr.ptr, fr.fs, fr.nf, fr.w, fr.h, scale, o.data_ptr())
    torch.cuda.synchronize()
    return light_words(o, fr.nf)


def planes_light(c, pl, sc, scale):
    """the eight words per frame of lumahip_planes_light_level_frames_device; pl: tests/support/device.py Planes"""
    import torch
    o = light_buf(pl.nf)
    c.planes_light_level_frames_device(pl.ptrs, pl.st, pl.pfs, pl.nf, pl.w, pl.h, pl.profile, sc, scale, o.data_ptr())
    torch.cuda.synchronize()
    return light_words(o, pl.nf)
