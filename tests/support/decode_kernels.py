"""What tests/test_gpu_decode_kernels.py and tests/test_decode_kernels_host.py share, numpy and the oracle alone: the matrix of the plain
decode with its table in LDS and the k_decode<CS, SUB, VW, GL = false, DISP = false, YT, RB, OUT16> instantiations it launches, the
source planes of a launch, the ORACLE's decode of them, where a call's frames lie in its output buffers, the comparison of those
buffers with the expectation, and wrong kernels modelled with the oracle and numpy, which every row's inputs must tell from a right one.

Nothing the library wrote enters an expectation.  Helpers here assert with an explicit message: pytest rewrites `assert` in test
modules only."""
import collections

import numpy as np

from tests.support import frame_kernels as fk
from tests.support.host import SENTINEL, float_to_half_np, plane_rows, same_bits

LUV, RGB, YCC, XYZ = fk.LUV, fk.RGB, fk.YCC, fk.XYZ
SIZES = [(64, 32), (264, 70), (258, 6), (6, 4)]   # VW 4, one tile / VW 4, several tiles both ways / VW 2, a ragged last tile / one unit row
SC_FAR = 3e5                                      # outside [2^-16, 2^16]: XformConst::sc_mode 2
SCS = (1.0, 20.0)
FLOAT_FORMS, HALF_FORMS = ("packed", "planar", "rotating"), ("packed", "planar")
# variant -> the tunes that make decode_impl pick it for a YCbCr quantizer; the other colour spaces have the plain kernels alone
VARIANTS = {"plain": (("ycbcr_tables", 0),), "yt": (("ycbcr_rb_tables", 0),), "rb": (("ycbcr_rb_tables", 2),)}
CASES = ((LUV, "plain"), (RGB, "plain"), (YCC, "plain"), (YCC, "yt"), (YCC, "rb"), (XYZ, "plain"))
MIN_DISTINCT = fk.MIN_DISTINCT
PAD, BASE = 4, 4                                  # elements behind every frame (planar: every plane) / in front of the first

Row = collections.namedtuple("Row", "id cs variant cfg tunes profile w h sc form out16")


def cfg_of(cs, profile):
    """PQ-11 for Lu'v', RGB and XYZ, PQ-10 YCbCr (maxLum 1000, colour depth 10); the 8-bit sibling for the 8-bit profiles"""
    if profile < 2:
        return fk.pq8(cs)
    return fk.config(cs, fk.PQ, 10 if cs == YCC else 11)


def tunes_of(cs, variant):
    return VARIANTS[variant] if cs == YCC else ()


def nframes(form):
    """three frames; four on the rotating rows, so that buffer 0 holds two (k = fu / 3 of dec_process reaches 1)"""
    return 4 if form == "rotating" else 3


def sc_mode(sc):
    """luma_device.hpp XformConst::sc_mode"""
    return 0 if sc == 1.0 else 1 if 2.0 ** -16 <= sc <= 2.0 ** 16 else 2


def _ident(cs, variant, out16, profile, w, h, sc, form):
    return "%s-%s-%s-p%d-%dx%d-sc%g-%s" % (fk.SPACES[cs][0], variant, "f16" if out16 else "f32", profile, w, h, sc, form)


def decode_matrix():
    """Rows of (id, cs, variant, cfg, tunes, profile, w, h, sc, form, out16): every (colour space, variant) by float and binary16
    frames, preScaling 1 and 20, both 16-bit profiles and the four sizes, the call form going round; behind them the 8-bit profiles
    -- one at 264x70, the other at 258x6 -- and, YCbCr only, one row with preScaling 3e5 at 258x6"""
    out = []

    def add(cs, variant, out16, profile, w, h, sc, form):
        out.append(Row(_ident(cs, variant, out16, profile, w, h, sc, form), cs, variant, cfg_of(cs, profile), tunes_of(cs, variant), profile,
                       w, h, sc, form, out16))

    for ci, (cs, variant) in enumerate(CASES):
        for out16 in (False, True):
            forms = HALF_FORMS if out16 else FLOAT_FORMS
            j = 0
            for sc in SCS:
                for profile in (2, 3):
                    for (w, h) in SIZES:
                        add(cs, variant, out16, profile, w, h, sc, forms[(ci + j + j // 4) % len(forms)])
                        j += 1
            for profile, (w, h) in zip((1, 0) if out16 else (0, 1), SIZES[1:3]):
                add(cs, variant, out16, profile, w, h, SCS[-1], forms[(ci + j) % len(forms)])
                j += 1
        if cs == YCC:
            add(cs, variant, variant == "yt", 2, 258, 6, SC_FAR, "planar" if variant == "yt" else "packed")
    return out


def kernel_of(cs, profile, w, out_aligned4, frame_stride, tunes, out16):
    """(CS, SUB, VW, YT, RB, OUT16) of the k_decode a device call launches for a quantizer whose table is in LDS
    (lumahip_decode.hip decode_impl): four pixels per thread need w % 4 == 0, every output pointer aligned to four elements and
    frame_stride % 4 == 0; the y table belongs to a YCbCr quantizer unless "ycbcr_tables" is 0; the red / blue tables need it and
    "ycbcr_rb_tables" not 0 (mode 1 leaves the launch to the lag policy: the matrix asks for mode 2 wherever it wants RB)"""
    t = dict(tunes)
    yt = cs == YCC and t.get("ycbcr_tables", 1) != 0
    rb = yt and t.get("ycbcr_rb_tables", 1) != 0
    return (cs, profile in (0, 2), 4 if (w % 4 == 0 and out_aligned4 and frame_stride % 4 == 0) else 2, yt, rb, bool(out16))


def all_kernels():
    """the 48 instantiations pick_dec<false> and pick_dec_f16 return from the device entry points for a table in LDS"""
    out = set()
    for (cs, variant) in CASES:
        for sub in (True, False):
            for vw in (4, 2):
                for out16 in (False, True):
                    out.add((cs, sub, vw, cs == YCC and variant != "plain", variant == "rb", out16))
    return out


# ---- where a call's frames lie
class OutLayout:
    """The output buffers of one decode call, in elements of its type (float32, or binary16 as uint16 bits): `base` elements in front of
    the first frame of every buffer, `pad` behind every frame (planar: behind every colour plane).
    packed    one buffer, frame f at base + f * fs, fs = 3 w h + pad
    planar    three buffers, colour plane c of frame f at buffer c's base + f * fs, fs = w h + pad
    rotating  three buffers, frame f packed at buffer f % 3's base + (f // 3) * fs, fs = 3 w h + pad"""

    def __init__(self, form, nf, w, h, out16, pad=PAD, base=BASE):
        self.form, self.nf, self.w, self.h, self.out16, self.pad, self.base = form, nf, w, h, bool(out16), pad, base
        self.dtype = np.dtype(np.uint16 if out16 else np.float32)
        self.n = w * h
        self.fs = (self.n if form == "planar" else 3 * self.n) + pad
        if form == "packed":
            counts = [nf]
        elif form == "planar":
            counts = [nf] * 3
        elif form == "rotating":
            counts = [(nf + 2 - k) // 3 for k in range(3)]
        else:
            raise ValueError("form: 'packed', 'planar' or 'rotating', not %r" % (form,))
        self.elements = [base + k * self.fs for k in counts]

    @property
    def aligned4(self):
        """every pointer of the call is aligned to four elements, given buffers that are"""
        return self.base % 4 == 0

    def at(self, f, c):
        """(buffer, element offset) of colour plane c of frame f"""
        if self.form == "packed":
            return 0, self.base + f * self.fs + c * self.n
        if self.form == "planar":
            return c, self.base + f * self.fs
        return f % 3, self.base + (f // 3) * self.fs + c * self.n

    def blank(self):
        """the buffers before a call: the sentinel in every byte"""
        return [np.full(n * self.dtype.itemsize, SENTINEL, dtype=np.uint8) for n in self.elements]

    def filled(self, frames):
        """the buffers a right call leaves for these (nf, 3, h, w) frames of the layout's type"""
        frames = np.asarray(frames)
        if frames.dtype != self.dtype or frames.shape != (self.nf, 3, self.h, self.w):
            raise ValueError("frames of %s %r, the layout has %s %r" % (frames.dtype, frames.shape, self.dtype, (self.nf, 3, self.h, self.w)))
        bufs = self.blank()
        for f in range(self.nf):
            for c in range(3):
                b, off = self.at(f, c)
                bufs[b].view(self.dtype)[off:off + self.n] = frames[f, c].ravel()
        return bufs


Written = collections.namedtuple("Written", "lay bufs")      # an OutLayout and the bytes of its buffers after a call


def _nan16(b):
    return ((b & 0x7C00) == 0x7C00) & ((b & 0x03FF) != 0)


def differ(got, want):
    """elementwise: not the same bits and not both NaN; float32 arrays, or binary16 as uint16 bits"""
    if want.dtype == np.uint16:
        return (got != want) & ~(_nan16(got) & _nan16(want))
    g, w = got.view(np.uint32), want.view(np.uint32)
    return (g != w) & ~(np.isnan(got) & np.isnan(want))


def frames_problem(got, exp):
    """None, or what is wrong with the buffers of a call (`got`: Written) that should hold the (nf, 3, h, w) frames `exp` -- float32, or
    uint16 bits of binary16: the first value that is not the expected one bit for bit (two NaN are the same), named by frame, channel,
    row and column with both values; or the first byte outside the frames that no longer holds the sentinel"""
    lay, bufs = got
    exp = np.asarray(exp)
    if exp.dtype != lay.dtype or exp.shape != (lay.nf, 3, lay.h, lay.w):
        return "the expectation is %s %r, the layout has %s %r" % (exp.dtype, exp.shape, lay.dtype, (lay.nf, 3, lay.h, lay.w))
    if [b.size for b in bufs] != [n * lay.dtype.itemsize for n in lay.elements]:
        return "buffers of %r bytes, the layout has %r elements" % ([b.size for b in bufs], lay.elements)
    outside = [np.ones(b.size, dtype=bool) for b in bufs]
    esz = lay.dtype.itemsize
    for f in range(lay.nf):
        for c in range(3):
            b, off = lay.at(f, c)
            outside[b][off * esz:(off + lay.n) * esz] = False
            g = bufs[b].view(lay.dtype)[off:off + lay.n].reshape(lay.h, lay.w)
            if not (np.array_equal(g, exp[f, c]) if lay.out16 else same_bits(g, exp[f, c])):      # (halves: below, for two NaN)
                bad = differ(g, exp[f, c])
                if not bad.any():
                    continue
                y, x = (int(v) for v in np.argwhere(bad)[0])
                fmt = "0x%04x" if lay.out16 else "%r (0x%08x)"
                one = (lambda a: fmt % int(a[y, x])) if lay.out16 else (lambda a: fmt % (a[y, x], int(a.view(np.uint32)[y, x])))
                return "frame %d channel %d row %d column %d: %s, expected %s (%d of %d values of this plane differ)" % (
                    f, c, y, x, one(g), one(exp[f, c]), int(bad.sum()), lay.n)
    for b in range(len(bufs)):
        changed = np.flatnonzero(outside[b] & (bufs[b] != SENTINEL))
        if changed.size:
            return "buffer %d: byte %d outside the frames holds 0x%02x, not the sentinel (%d such bytes)" % (b, int(changed[0]),
                                                                                                    int(bufs[b][changed[0]]), changed.size)
    return None


# ---- the planes of a launch
PLANTED_COLUMNS = 16
PLANTED_ROWS = {(264, 70): 8, (258, 6): 4}   # luma rows of the corner that holds the boundary and out-of-range codes


def planted_codes(cfg, profile):
    """0, 1, maxVal - 1, maxVal, maxVal + 1, maxC, maxC + 1 and all ones, where the sample holds them"""
    top, topc, ones = (1 << cfg[1]) - 1, (1 << cfg[3]) - 1, 0xFFFF if profile > 1 else 0xFF
    return sorted({v for v in (0, 1, top - 1, top, top + 1, topc, topc + 1, ones) if v <= ones})


def plane_values(plane, profile):
    """the integers of a (rows, row bytes) plane without padding"""
    a = np.ascontiguousarray(plane)
    return (a.view("<u2") if profile > 1 else a).astype(np.int64)


def plane_of(values, profile):
    """the (rows, row bytes) plane of a (rows, columns) array of integers"""
    rows = values.shape[0]
    return np.ascontiguousarray(values.astype("<u2" if profile > 1 else np.uint8)).view(np.uint8).reshape(rows, -1)


def _picture_values(rng, cfg, profile, w, h):
    """smooth code fields with a little noise, as _picture_codes of tests/test_gpu_rb_tables.py makes them, scaled to the code range:
    neighbouring pixels, neighbouring codes -- what rb_wave_local calls local"""
    ones = 0xFFFF if profile > 1 else 0xFF
    ty, tc = min((1 << cfg[1]) - 1, ones), min((1 << cfg[3]) - 1, ones)
    yy, xx = np.mgrid[0:h, 0:w]
    y = ty * (0.49 + 0.37 * np.sin(xx / 97.0) * np.cos(yy / 61.0)) + rng.normal(0, 6 * ty / 1023.0, (h, w))
    ch, cw = (h // 2, w // 2) if profile in (0, 2) else (h, w)
    cy, cx = np.mgrid[0:ch, 0:cw]
    cb = tc * (0.5 + 0.156 * np.sin(cx / 53.0 + 1.0)) + rng.normal(0, 2 * tc / 1023.0, (ch, cw))
    cr = tc * (0.5 + 0.156 * np.cos(cy / 47.0)) + rng.normal(0, 2 * tc / 1023.0, (ch, cw))
    return [np.clip(np.rint(a), 0, t).astype(np.int64) for a, t in ((y, ty), (cb, tc), (cr, tc))]


_src = {}


def source_planes(cfg, profile, w, h, nf, picture=False):
    """nf distinct frames of code planes, each three (rows, row bytes) arrays: seeded in-range codes -- luma 0 .. 2^bitdepth - 1, chroma
    0 .. 2^bitdepthC - 1, as far as the sample holds them -- or, `picture`, smooth fields in every frame but frame 1.  At 264x70 the
    8x16 corner, and at 258x6 a 4x16 corner, hold planted_codes going round differently in every plane and frame: a chroma code
    beyond maxC sends Lu'v' chroma, the YT tables' `bad` and RB's `redo` to the complete functions.  Made once per key, read-only"""
    key = (cfg, profile, w, h, nf, picture)
    if key not in _src:
        ones, frames = 0xFFFF if profile > 1 else 0xFF, []
        codes = np.array(planted_codes(cfg, profile))
        for f in range(nf):
            rng = np.random.default_rng([cfg[0], cfg[1], cfg[2], cfg[3], profile, w, h, f, int(picture)])
            if picture and f % 3 != 1:
                vals = _picture_values(rng, cfg, profile, w, h)
            else:
                vals = []
                for p in range(3):
                    rows, rb = plane_rows(w, h, profile, p)
                    vals.append(rng.integers(0, min(1 << (cfg[1] if p == 0 else cfg[3]), ones + 1), size=(rows, rb // (2 if profile > 1 else 1))))
            fr = []
            for p in range(3):
                v = vals[p]
                if (w, h) in PLANTED_ROWS:
                    sub = 2 if (p and profile in (0, 2)) else 1
                    cr, cc = PLANTED_ROWS[(w, h)] // sub, PLANTED_COLUMNS // sub
                    r, c = np.mgrid[0:cr, 0:cc]
                    v[:cr, :cc] = codes[(5 * r + c + f + 3 * p) % codes.size]
                a = plane_of(v, profile)
                a.setflags(write=False)
                fr.append(a)
            frames.append(fr)
        _src[key] = frames
    return _src[key]


def is_picture(row):
    """the rb rows at 264x70 decode picture-like planes in two of their frames"""
    return row.variant == "rb" and (row.w, row.h) == (264, 70)


def chroma_out_of_range(row, s):
    """whether the planes hold a chroma code beyond maxC that the colour space gives to a complete function (RGB and XYZ read all
    three planes through the table, whose read clamps)"""
    if row.cs not in (LUV, YCC):
        return False
    return any((plane_values(fr[p], row.profile) > (1 << row.cfg[3]) - 1).any() for fr in s for p in (1, 2))


Expect = collections.namedtuple("Expect", "s frames want")
_exp = {}


def narrowed(frames):
    """float32 -> the uint16 bits of binary16, round to nearest even"""
    return float_to_half_np(frames).reshape(np.shape(frames))


def _decode(o, cfg, planes, profile, w, h, sc):
    st = [plane_rows(w, h, profile, p)[1] for p in range(3)]
    with np.errstate(all="ignore"):
        return np.stack([fk.oracle(o, cfg).decode(fr, st, w, h, sc, profile) for fr in planes])


def expected(o, row):
    """The inputs of a row's launch and what the oracle makes of them, computed once per key and not written to afterwards:
    s       source_planes of the row
    frames  Oracle.decode of every frame's planes: (nf, 3, h, w) float32
    want    what the call's buffers are held to: frames, or on a binary16 row float_to_half_np of them"""
    nf, picture = nframes(row.form), is_picture(row)
    key = (row.cfg, row.profile, row.w, row.h, row.sc, nf, picture, row.out16)
    if key not in _exp:
        s = source_planes(row.cfg, row.profile, row.w, row.h, nf, picture)
        frames = _decode(o, row.cfg, s, row.profile, row.w, row.h, row.sc)
        want = narrowed(frames) if row.out16 else frames
        for a in (frames, want):
            a.setflags(write=False)
        _exp[key] = Expect(s, frames, want)
    return _exp[key]


def informative(exp, tag):
    """asserted on the reference alone -- (nf, 3, h, w) float32, or uint16 bits of binary16: every channel of every frame holds at least
    MIN_DISTINCT distinct finite values (6x4 has 24 pixels: exempt), the three channels of a frame differ from each other, and so do
    the frames of a launch.  Returns the smallest count"""
    exp = np.asarray(exp)
    nf, _, h, w = exp.shape
    halves = exp.dtype == np.uint16
    bits = exp if halves else exp.view(np.uint32)
    finite = ((exp & 0x7C00) != 0x7C00) if halves else np.isfinite(exp)
    least = None
    for f in range(nf):
        for c in range(3):
            n = np.unique(bits[f, c][finite[f, c]]).size
            least = n if least is None else min(least, n)
            assert w * h <= 24 or n >= MIN_DISTINCT, tag + (f, c, "%d distinct finite values" % n)
            for d in range(c + 1, 3):
                assert not np.array_equal(bits[f, c], bits[f, d]), tag + (f, "channels %d and %d are the same" % (c, d))
        for g in range(f + 1, nf):
            assert not np.array_equal(bits[f], bits[g]), tag + ("frames %d and %d are the same" % (f, g),)
    return least


# ---- wrong kernels, modelled with the oracle and numpy alone
def truncated(frames):
    """float32 -> the uint16 bits of binary16 with the excess bits dropped: where rounding to nearest went away from zero, one back"""
    frames = np.asarray(frames, dtype=np.float32)
    b = narrowed(frames)
    with np.errstate(all="ignore"):
        up = np.isfinite(frames) & (np.abs(b.view(np.float16).astype(np.float64)) > np.abs(frames.astype(np.float64)))
    return (b - up.astype(np.uint16)).astype(np.uint16)


def _rolled(plane, profile):
    """a chroma plane whose samples each come from the quad to the left (the first from the last)"""
    return plane_of(np.roll(plane_values(plane, profile), 1, axis=1), profile)


def wrong_kernels(o, row):
    """{name: frames}: what kernels with one fault each would write for this row's source planes, in the type of `expected`'s want.
    Only the faults that apply to the row are modelled:
    uv_swapped       the second and third plane change places
    frames_swapped   frames 0 and 1 change places
    sc_dropped       no `/ sc` (rows with sc != 1)
    neighbour_quad   4:2:0: every chroma sample taken from the quad to the left
    chroma_clamped   a chroma code beyond maxC clamped to it instead of given to the complete function (rows whose planes hold one)
    last_column      the luma codes of the last column off by one
    truncated        binary16 rows: narrowed by dropping bits instead of rounding to nearest even"""
    ex = expected(o, row)
    profile, w, h = row.profile, row.w, row.h
    dec = lambda planes, sc=row.sc: _decode(o, row.cfg, planes, profile, w, h, sc)      # noqa: E731
    fin = narrowed if row.out16 else (lambda a: a)
    nf = len(ex.s)
    out = {"uv_swapped": fin(dec([[fr[0], fr[2], fr[1]] for fr in ex.s])),
           "frames_swapped": np.ascontiguousarray(ex.want[[1, 0] + list(range(2, nf))])}
    if row.sc != 1.0:
        out["sc_dropped"] = fin(dec(ex.s, 1.0))
    if profile in (0, 2):
        out["neighbour_quad"] = fin(dec([[fr[0], _rolled(fr[1], profile), _rolled(fr[2], profile)] for fr in ex.s]))
    if chroma_out_of_range(row, ex.s):
        topc = (1 << row.cfg[3]) - 1
        out["chroma_clamped"] = fin(dec([[fr[0]] + [plane_of(np.minimum(plane_values(fr[p], profile), topc), profile) for p in (1, 2)] for fr in ex.s]))
    top = (1 << row.cfg[1]) - 1
    moved = []
    for fr in ex.s:
        v = plane_values(fr[0], profile)
        v[:, -1] += np.where(v[:, -1] < top, 1, -1)
        moved.append([plane_of(v, profile), fr[1], fr[2]])
    out["last_column"] = fin(dec(moved))
    if row.out16:
        out["truncated"] = truncated(ex.frames)
    return out


def applies(name, kernel):
    """whether a kernel (CS, SUB, VW, YT, RB, OUT16) has the code the named fault of wrong_kernels is a fault of"""
    cs, sub, _, _, _, out16 = kernel
    return {"neighbour_quad": sub, "chroma_clamped": cs in (LUV, YCC), "truncated": out16}.get(name, True)


def layout_of(row):
    return OutLayout(row.form, nframes(row.form), row.w, row.h, row.out16)


def tells(o, row, frames):
    """whether the row's comparison fails for a kernel that writes `frames`"""
    lay = layout_of(row)
    return frames_problem(Written(lay, lay.filled(frames)), expected(o, row).want) is not None


def row_kernel(row):
    """the kernel the row's launch takes, from the layout its call is given"""
    lay = layout_of(row)
    return kernel_of(row.cs, row.profile, row.w, lay.aligned4, lay.fs, row.tunes, row.out16)


__all__ = ["CASES", "FLOAT_FORMS", "HALF_FORMS", "SC_FAR", "SIZES", "VARIANTS", "Expect", "OutLayout", "Row", "Written", "all_kernels", "applies",
           "cfg_of", "chroma_out_of_range", "decode_matrix", "differ", "expected", "frames_problem", "informative", "is_picture", "kernel_of", "layout_of",
           "narrowed", "nframes", "plane_of", "plane_values", "planted_codes", "row_kernel", "sc_mode", "source_planes", "tells", "truncated",
           "tunes_of", "wrong_kernels"]
