"""Frames and code planes that lie beyond 2^31 and 2^32 elements or bytes of the pointer a call is given: the layouts, their arithmetic,
the sparse device buffers that hold them, the matrix of tests/test_gpu_far_layouts.py, its expectations (the oracle's; numpy's for the
words) and the wrong kernels tests/test_far_layouts_host.py models on a sparse picture of an allocation.

Every address the kernels form is base + frame term + row term + unit term.  A far layout makes the frame term (f * frame stride) or the
row term (row * stride) exceed 32 bits while the samples themselves stay a few hundred KB: the allocation is filled with the sentinel on
the device and only the samples are ever copied either way.

The layouts
  frames "far"     packed frames fs = 2^31 + 2 * 3wh elements apart (even, and a multiple of 4 where the vector loads of four need it):
                   frame 1 starts at >= 2^31 elements, frame 2 at >= 2^32.  Floats: about 24 GiB, halves: about 12 GiB.
  frames "rot"     the rotating decode: three buffers in one allocation, frame f at rot[f % 3] + (f // 3) * fs with the same fs; four
                   frames, so that buffer 0 holds two -- it lies behind the other two, 3wh + 4 elements apart, because the call refuses
                   buffers whose spans overlap.  Its frame 3 is beyond 2^31 elements, none beyond 2^32.  About 16 GiB.
  frames "planar3" three colour planes in three allocations of 2^32 bytes and more each, so that the pointer DIFFERENCES exceed 2^32 on
                   their own; the frame stride stays compact (w h + 4): far strides in three float allocations would take 72 GiB.
  planes "far16"   one allocation, plane p at lead + p * STAGGER, pfs[p] = 2^31 + 16 (p + 1) bytes, rows row bytes + 16 apart: every base,
                   stride and frame stride takes the vector accesses (read_planes: aligned 1).  About 6 GiB.
  planes "farodd"  the same with odd bases, odd row strides and pfs[p] = 2^31 + 1 + 2 p: aligned 0, the byte-wise branches of
                   load_samples / store_samples.
  planes "wide"    ONE frame whose rows are 2^e + 64 bytes apart, e the smallest exponent that puts the last luma row beyond 2^32 bytes
                   (2^26 at 70 and 72 rows: rows 32 and up beyond 2^31, rows 64 and up beyond 2^32; 2^28 at 18 rows).  Profile 3 gives the
                   chroma planes as many rows.  About 6.5 GiB.
  planes "wideodd" the same with 2^e + 65 and odd bases: the byte-wise branch.
  image "fardisp"  the RGBA output of the display decode: the pitch of "wide" and a frame stride of h pitches + 4096 bytes, beyond 2^32.
                   About 15 GiB.

The lead.  `.ptr` / `.ptrs` lie LEAD = 2^31 elements (frames) or bytes (planes) into their allocation.  A kernel that narrowed a term to 32
bits would form base + (term mod 2^32) -- unsigned -- or base + (int32) term -- signed.  Both stay inside the allocation, the signed one
thanks to the lead (it is at most 2^31 below the base), and both differ from the true address wherever the term does not fit: the signed
one from 2^31 on, the unsigned one from 2^32 on.  So a wrong kernel fails the comparison and leaves no allocation.  No row here needed a
smaller lead: the largest allocation (float frames, 24 GiB) is half the cap of 48 GiB live at once.

Helpers here assert with an explicit message: pytest rewrites `assert` in test modules only."""
import collections

import numpy as np

from tests.support import frame_kernels as fk
from tests.support import light_level as ll
from tests.support import measuring as ms
from tests.support import plane_kernels as pk
from tests.support import transcode_half as th
from tests.support.display import DISPLAY_SETS, display_bytes, display_frames, display_t
from tests.support.host import CFG, SENTINEL, float_to_half_np, plane_rows, same_bits, widen_halves
from tests.support.moments import MOM_BLOCKS
from tests.support.planes_measure import case_rng, two_sets

GIB = 1 << 30
CAP = 48 * GIB            # device memory live at once, at most
CHUNK = 256 << 20         # the piece the sentinel checks look at at a time
LEAD = 1 << 31            # elements in front of far frames, bytes in front of far planes
STAGGER = 1 << 16         # bytes between the planes of a set in its one allocation (the largest plane here: 72 rows of 544 bytes)
SLACK = 4096              # bytes behind the last sample of an allocation
PAD = 4                   # elements behind a compact frame or colour plane (tests/support/device.py Frames)
PLANAR3_BYTES = 1 << 32   # what each allocation of "planar3" holds at least
SIZES = ((264, 70), (34, 18))
HALF_SIZES = ((264, 72), (36, 20))
FRAME_KINDS = ("far", "rot", "planar3")
PLANE_KINDS = ("far16", "farodd", "wide", "wideodd")
LUV, YCC = CFG["pq11_luv8"], CFG["pq10_ycbcr10"]
FORMS = ("packed", "planar", "f16", "planar_f16")
SUFFIX = {"packed": "", "planar": "_planar", "f16": "_f16", "planar_f16": "_planar_f16"}
LIGHT_SCALE = 20.0


def u32(off):
    """what an unsigned 32-bit computation makes of a term"""
    return off & 0xFFFFFFFF


def s32(off):
    """... and a signed one"""
    return ((off + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


NARROW = {None: lambda x: x, "u32": u32, "s32": s32}


# ---- the arithmetic of the layouts (no torch, no library)
FramesLayout = collections.namedtuple("FramesLayout", "kind nf n3 esz fs lead bases alloc")
PlanesLayout = collections.namedtuple("PlanesLayout", "kind nf profile rows rb st pfs lead off alloc")


def frames_layout(kind, w, h, nf, esz):
    """frame f at element bases[f % len(bases)] + (f // len(bases)) * fs of an allocation of `alloc` elements"""
    n3 = 3 * w * h
    fs = (1 << 31) + 2 * n3
    if kind == "far":
        return FramesLayout(kind, nf, n3, esz, fs, LEAD, (LEAD,), LEAD + (nf - 1) * fs + n3 + SLACK)
    if kind == "rot":
        if nf != 4:
            raise ValueError("the rotating layout: four frames")
        bases = (LEAD + 2 * (n3 + PAD), LEAD, LEAD + n3 + PAD)      # (buffer 0, which holds two frames, behind the other two)
        return FramesLayout(kind, nf, n3, esz, fs, LEAD, bases, bases[0] + fs + n3 + SLACK)
    raise ValueError(kind)


def frame_offset(fl, f, narrow=None):
    """the element of the allocation frame f begins at, the frame term narrowed as `narrow` says"""
    nb = len(fl.bases)
    return fl.bases[f % nb] + NARROW[narrow]((f // nb) * fl.fs)


def wide_exponent(rows):
    e = 20
    while (rows - 1) << e < (1 << 32):
        e += 1
    return e


def planes_layout(kind, w, h, profile, nf):
    """plane p of frame f at byte off[p] + f * pfs[p] of ONE allocation of `alloc` bytes, rows st[p] apart"""
    rows, rb = zip(*[plane_rows(w, h, profile, p) for p in range(3)])
    odd = kind in ("farodd", "wideodd")
    if kind in ("far16", "farodd"):
        st = fk.odd_layout(w, h, profile)[0] if odd else fk.wide_layout(w, h, profile)
        pfs = tuple((1 << 31) + (1 + 2 * p if odd else 16 * (p + 1)) for p in range(3))
    elif kind in ("wide", "wideodd"):
        st = ((1 << wide_exponent(rows[0])) + (65 if odd else 64),) * 3
        pfs = tuple(rows[p] * st[p] for p in range(3))
    else:
        raise ValueError(kind)
    off = tuple(LEAD + p * STAGGER + (1 if odd else 0) for p in range(3))
    end = max(off[p] + (nf - 1) * pfs[p] + (rows[p] - 1) * st[p] + rb[p] for p in range(3))
    return PlanesLayout(kind, nf, profile, rows, rb, tuple(st), pfs, LEAD, off, end + SLACK)


DispLayout = collections.namedtuple("DispLayout", "nf w h st dfs lead alloc")


def disp_layout(w, h, nf):
    """the RGBA image of the display decode with a wide pitch AND a far frame stride: row r of frame f at byte lead + f * dfs + r * st of
    one allocation, st = 2^e + 64 as the wide planes' (rows beyond 2^31 and beyond 2^32), dfs = h * st + 4096 (frames 1 and 2 beyond 2^32)"""
    st = (1 << wide_exponent(h)) + 64
    dfs = h * st + 4096
    return DispLayout(nf, w, h, st, dfs, LEAD, LEAD + (nf - 1) * dfs + (h - 1) * st + 4 * w + SLACK)


def disp_offset(dl, f, r, narrow_frame=None, narrow_row=None):
    return dl.lead + NARROW[narrow_frame](f * dl.dfs) + NARROW[narrow_row](r * dl.st)


def row_offset(pl, p, f, r, narrow_frame=None, narrow_row=None):
    """the byte of the allocation row r of plane p of frame f begins at, either term narrowed"""
    return pl.off[p] + NARROW[narrow_frame](f * pl.pfs[p]) + NARROW[narrow_row](r * pl.st[p])


# ---- the library's host checks, restated
def check_layout_ok(w, h, profile, nf, st, pfs):
    """lumahip_core.hip check_layout without its colour-plane test"""
    for p in range(3):
        rows, rb = plane_rows(w, h, profile, p)
        if st[p] < rb or st[p] >= (1 << 31) or (nf > 1 and pfs[p] < rows * st[p]):
            return False
    return True


def colour_planes_ok(ptrs, esz, fs, nf, n):
    """check_layout's colour-plane test: byte pointers of the three colour planes, fs and n = w h in elements"""
    if nf > 1 and fs < n:
        return False
    span = (nf - 1) * fs + n
    for i in range(3):
        for j in range(i + 1, 3):
            d = abs(ptrs[i] - ptrs[j]) // esz
            if not (d >= span or (d >= n and (nf == 1 or d + n <= fs))):
                return False
    return True


def frame_alignment(ptrs, esz, fs, w):
    """lumahip_internal.hpp check_frame_alignment: (accepted, al4)"""
    def al(n):
        return all(q % (n * esz) == 0 for q in ptrs) and fs % n == 0
    return al(2), w % 4 == 0 and al(4)


def planes_aligned(ptrs, st, pfs, profile, vw):
    """lumahip_internal.hpp planes_aligned: what read_planes puts into DecArgs::aligned"""
    sub, bps = profile in (0, 2), 2 if profile > 1 else 1
    for k in range(3):
        ub = (vw // 2 if (k and sub) else vw) * bps
        if ptrs[k] % ub or st[k] % ub or pfs[k] % ub:
            return False
    return True


def ranges_overlap(a, na, b, nb):
    return a < b + nb and b < a + na


def plane_extent(w, h, profile, p, st, pfs, nf, narrow=None):
    """lumahip_internal.hpp plane_extent; narrow: the sum as a 32-bit host computation would form it"""
    rows, rb = plane_rows(w, h, profile, p)
    return NARROW[narrow]((nf - 1) * pfs + (rows - 1) * st + rb)


def frame_span_bytes(w, h, fs, nf, esz, narrow=None):
    """check_out_overlap's frame_span"""
    return NARROW[narrow](((nf - 1) * fs + w * h) * esz)


# ---- the refusals that must still refuse: where their arguments lie, and what the host checks make of them
REFUSALS = ("words_in_far_frame_2", "words_in_last_wide_row", "target_over_far_frame_2", "pfs_below_wide_plane")
REFUSAL_SIZE = (264, 70)


def refusal_args(name):
    """the numbers of a refusal, offsets counted in bytes from the start of the one allocation all of its arguments lie in"""
    w, h = REFUSAL_SIZE
    if name == "words_in_far_frame_2":          # lumahip_distortion_frames_device: out_dev 32 bytes into colour plane 0 of frame 2
        fl = frames_layout("far", w, h, 3, 4)
        return dict(fl=fl, ptr=fl.lead * 4, out=(fl.lead + 2 * fl.fs + 8) * 4, out_bytes=3 * 12 * 8, alloc=fl.alloc * 4)
    if name == "words_in_last_wide_row":        # lumahip_planes_light_level_frames_device: out_dev 8 bytes into the last luma row
        pl = planes_layout("wide", w, h, 3, 1)
        return dict(pl=pl, out=pl.off[0] + (pl.rows[0] - 1) * pl.st[0] + 8, out_bytes=8 * 8, alloc=pl.alloc)
    if name == "target_over_far_frame_2":       # lumahip_transcode_frames_device: the last 64 .. 79 bytes of target plane p in source frame 2
        pl = planes_layout("far16", w, h, 2, 3)
        st = fk.wide_layout(w, h, 2)
        tpfs = [pl.rows[p] * st[p] + 48 for p in range(3)]
        ext = [plane_extent(w, h, 2, p, st[p], tpfs[p], 3) for p in range(3)]
        dst = [pl.off[p] + 2 * pl.pfs[p] - (ext[p] - 64) // 16 * 16 for p in range(3)]
        return dict(pl=pl, st=st, tpfs=tpfs, ext=ext, dst=dst, alloc=pl.alloc)
    if name == "pfs_below_wide_plane":          # lumahip_planes_light_level_frames_device, two frames: pfs one row short of a plane
        pl = planes_layout("wide", w, h, 3, 2)
        return dict(pl=pl, pfs=[pl.pfs[p] - pl.st[p] for p in range(3)], alloc=pl.alloc)
    raise ValueError(name)


def refusal_facts(name, narrow=None):
    """(refused, inside): what the library's check -- with `narrow`, a check that forms its span in 32 bits -- decides, and whether
    everything a launch would touch if the call were accepted lies inside the allocation"""
    w, h = REFUSAL_SIZE
    a = refusal_args(name)
    if name == "words_in_far_frame_2":
        span = frame_span_bytes(w, h, a["fl"].fs, 3, 4, narrow)
        refused = any(ranges_overlap(a["out"], a["out_bytes"], a["ptr"] + k * w * h * 4, span) for k in range(3))
        return refused, a["out"] + a["out_bytes"] <= a["alloc"]
    if name == "words_in_last_wide_row":
        pl = a["pl"]
        refused = any(ranges_overlap(a["out"], a["out_bytes"], pl.off[p], plane_extent(w, h, 3, p, pl.st[p], pl.pfs[p], 1, narrow)) for p in range(3))
        return refused, a["out"] + a["out_bytes"] <= a["alloc"]
    if name == "target_over_far_frame_2":
        pl = a["pl"]
        refused = any(ranges_overlap(pl.off[i], plane_extent(w, h, 2, i, pl.st[i], pl.pfs[i], 3, narrow), a["dst"][j], a["ext"][j])
                      for i in range(3) for j in range(3))
        return refused, all(pl.lead <= a["dst"][p] and a["dst"][p] + a["ext"][p] <= a["alloc"] for p in range(3))
    pl = a["pl"]
    refused = any(a["pfs"][p] < NARROW[narrow](pl.rows[p] * pl.st[p]) for p in range(3))
    return refused, all(pl.off[p] + a["pfs"][p] + (pl.rows[p] - 1) * pl.st[p] + pl.rb[p] <= a["alloc"] for p in range(3))


# ---- a sparse picture of an allocation: regions over a sentinel background
class Sparse:
    def __init__(self, size):
        self.size, self.regions = size, {}

    def write(self, at, data):
        data = np.ascontiguousarray(data).view(np.uint8).ravel()
        assert 0 <= at and at + data.size <= self.size, "a write outside the allocation: %d + %d of %d" % (at, data.size, self.size)
        self.regions[at] = data.copy()

    def read(self, at, n):
        assert 0 <= at and at + n <= self.size, "a read outside the allocation: %d + %d of %d" % (at, n, self.size)
        out = np.full(n, SENTINEL, dtype=np.uint8)
        for s, d in self.regions.items():
            lo, hi = max(s, at), min(s + d.size, at + n)
            if lo < hi:
                out[lo - at:hi - at] = d[lo - s:hi - s]
        return out


def put_frames(fl, frames, dtype, narrow=None):
    """the Sparse picture of frames in a frames layout, as a writer leaves it whose frame term is narrowed"""
    m = Sparse(fl.alloc * fl.esz)
    for f in range(fl.nf):
        m.write(frame_offset(fl, f, narrow) * fl.esz, np.asarray(frames[f]).astype(dtype))
    return m


def get_frames(m, fl, w, h, dtype, narrow=None):
    """the frames a reader finds whose frame term is narrowed: (nf, 3, h, w)"""
    return np.stack([m.read(frame_offset(fl, f, narrow) * fl.esz, fl.n3 * fl.esz).view(dtype).reshape(3, h, w) for f in range(fl.nf)])


def put_planes(pl, frames, narrow_frame=None, narrow_row=None):
    m = Sparse(pl.alloc)
    for f in range(pl.nf):
        for p in range(3):
            for r in range(pl.rows[p]):
                m.write(row_offset(pl, p, f, r, narrow_frame, narrow_row), np.asarray(frames[f][p])[r, :pl.rb[p]])
    return m


def get_planes(m, pl, narrow_frame=None, narrow_row=None):
    """the frames of tight (rows, row bytes) planes a reader finds"""
    return [[np.stack([m.read(row_offset(pl, p, f, r, narrow_frame, narrow_row), pl.rb[p]) for r in range(pl.rows[p])]) for p in range(3)]
            for f in range(pl.nf)]


# ---- the matrix
Row = collections.namedtuple("Row", "id group entry symbol form a b w h cs profile stats block shape nf")
# the entry points the matrix leaves out, and why
EXEMPT = {
    "lumahip_time_launches": "a timing loop over lumahip_encode_frames_device's own launch: nothing to compare, and it runs for seconds",
    "lumahip_probe_decode_traffic_device": "a traffic probe: it reports a bandwidth and is held to no reference",
    "lumahip_probe_encode_traffic_device": "a traffic probe: it reports a bandwidth and is held to no reference",
    "lumahip_decode_frames_device_ring": "hands its arguments to lumahip_decode_frames_device_rotating with bases and a frame stride "
                                         "the library chose (lumahip_decoded_ring_create): the caller cannot make them far",
    "lumahip_multi_encode_frames_device": "one lumahip_encode_frames_device per shard: needs several GPUs, the same kernels and checks",
    "lumahip_multi_decode_frames_device": "one lumahip_decode_frames_device per shard: needs several GPUs, the same kernels and checks",
}


def strided_symbols(capi):
    """every device entry point of the three ABI tables that takes a frame stride or plane frame strides: a size_t[3] among its
    parameters (plane frame strides), or a size_t in front of three unsigned (frame stride, nframes, w, h); the array calls and the
    probes take a size_t count and one unsigned at most"""
    import ctypes as C
    out = []
    for table in (capi._ABI, capi._ABI_MEASURE, capi._ABI_COMPARE):
        for name, (_, args) in table.items():
            if "_device" not in name and name != "lumahip_time_launches":
                continue
            if C.POINTER(C.c_size_t) in args or (C.c_size_t in args and args.count(C.c_uint) >= 3):
                out.append(name)
    return out


def cfg_of(cs, profile):
    """the quantizer of a row: PQ-11 Lu'v' 8 or PQ-10 YCbCr 10; the 8-bit profiles take their PQ-8 siblings (a sample holds 8 bits)"""
    if profile < 2:
        return fk.pq8(fk.LUV if cs == "luv" else fk.YCC)
    return LUV if cs == "luv" else YCC


def _variants(i, sizes=SIZES):
    """the (w, h, cs, profile) one (entry point, layout) runs at: both sizes under PQ-11 Lu'v', profiles 2 and 3 changing places from one
    layout to the next, and the larger size under PQ-10 YCbCr"""
    pa, pb = ((2, 3), (3, 2))[i % 2]
    return [sizes[0] + ("luv", pa), sizes[1] + ("luv", pb), sizes[0] + ("ycc", pa)]


def matrix():
    """every row of tests/test_gpu_far_layouts.py.  a / b: the layouts of the call's first and second operand ("compact", a FRAME_KINDS or
    a PLANE_KINDS name)"""
    rows = []

    def add(group, entry, symbol, form, a, b, w, h, cs, profile, stats=False, block=None, shape="default", nf=None):
        wide = a in ("wide", "wideodd") or b in ("wide", "wideodd")
        nf = nf if nf is not None else 4 if b == "rot" else 1 if wide else 3
        ident = "%s-%s-%s-%dx%d-%s-p%d%s%s%s" % (symbol.replace("lumahip_", "").replace("_frames_device", ""), a, b, w, h, cs, profile,
                                                 "-stats" if stats else "", "-b%d" % block if block is not None else "", "" if shape == "default" else "-" + shape)
        rows.append(Row(ident, group, entry, symbol, form, a, b, w, h, cs, profile, stats, block, shape, nf))

    n = 0
    # 1. encode
    enc = [(form, "planar3" if form.startswith("planar") else "far", "compact") for form in FORMS]
    enc += [("packed", "compact", k) for k in PLANE_KINDS]
    for i, (form, a, b) in enumerate(enc):
        sym = "lumahip_encode_frames_device" + SUFFIX[form]
        for j, (w, h, cs, profile) in enumerate(_variants(i)):
            add("encode", "encode", sym, form, a, b, w, h, cs, profile, stats=(i + j) % 2 == 0)
        if b == "compact" or (form == "packed" and b == "far16"):
            add("encode", "encode", sym, form, a, b, 264, 70, "luv", 0, stats=True)
    # 2. decode
    dec = [("packed", k, "compact") for k in PLANE_KINDS]
    dec += [("packed", "compact", "far"), ("planar", "compact", "planar3"), ("rotating", "compact", "rot"), ("f16", "compact", "far"),
            ("planar_f16", "compact", "planar3")]
    for i, (form, a, b) in enumerate(dec):
        sym = "lumahip_decode_frames_device" + {"rotating": "_rotating"}.get(form, SUFFIX.get(form, ""))
        for (w, h, cs, profile) in _variants(i):
            add("decode", "decode", sym, form, a, b, w, h, cs, profile)
        if a == "far16" or a == "compact":
            add("decode", "decode", sym, form, a, b, 264, 70, "luv", 0)
    # ... and the display form: far and wide planes into a compact image, compact planes into an image with a wide pitch and a far
    # frame stride; `block` is the index of the parameter set (tests/support/display.py DISPLAY_SETS)
    for i, (a, b) in enumerate([("far16", "compact"), ("wide", "compact"), ("compact", "fardisp")]):
        for j, (w, h, cs, profile) in enumerate(_variants(i)):
            add("display", "display", "lumahip_decode_display_frames_device", None, a, b, w, h, cs, profile, block=(i + j) % len(DISPLAY_SETS))
    add("display", "display", "lumahip_decode_display_frames_device", None, "far16", "compact", 264, 70, "luv", 0, block=3)
    # 3. transcode and transcode-half
    two = [("far16", "compact"), ("compact", "far16"), ("far16", "farodd"), ("farodd", "far16"), ("wide", "compact"), ("compact", "wide"),
           ("wideodd", "compact"), ("compact", "wideodd")]
    for entry, sym, sizes in (("transcode", "lumahip_transcode_frames_device", SIZES), ("half", "lumahip_transcode_half_frames_device", HALF_SIZES)):
        for i, (a, b) in enumerate(two):
            for j, (w, h, cs, profile) in enumerate(_variants(i, sizes)):
                add("transcode", entry, sym, None, a, b, w, h, cs, profile, stats=(i + j) % 2 == 1)
        add("transcode", entry, sym, None, "far16", "compact", sizes[0][0], sizes[0][1], "luv", 0, stats=True)
        add("transcode", entry, sym, None, "compact", "far16", sizes[0][0], sizes[0][1], "luv", 0)
    # 4. the frame-fed measuring calls: every form on far frames, and on compact frames with one kind of far given planes -- the kinds
    # go round the forms, so that each family meets each kind
    fam_blocks = {"distortion": (None,), "distortion_map": (16, 32, 64), "moments_map": MOM_BLOCKS}
    for k, fam in enumerate(ms.FAMILIES):
        for j, form in enumerate(FORMS):
            sym = "lumahip_%s_frames_device%s" % (fam, SUFFIX[form])
            cases = [("planar3" if form.startswith("planar") else "far", "compact"), ("compact", PLANE_KINDS[(j + k) % 4])]
            for i, (a, b) in enumerate(cases):
                for (w, h, cs, profile) in _variants(i + j):
                    n += 1
                    add("measure", fam, sym, form, a, b, w, h, cs, profile, block=fam_blocks[fam][n % len(fam_blocks[fam])])
            add("measure", fam, sym, form, cases[0][0], "compact", 264, 70, "luv", 0, block=fam_blocks[fam][0])
    # 5. the transcode measuring calls
    for fam, sym in (("distortion", "lumahip_transcode_distortion_frames_device"), ("distortion_map", "lumahip_transcode_distortion_map_frames_device"),
                     ("moments_map", "lumahip_transcode_moments_map_frames_device")):
        for i, (a, b) in enumerate([("far16", "compact"), ("compact", "far16"), ("far16", "farodd"), ("wide", "wideodd")]):
            for (w, h, cs, profile) in _variants(i):
                n += 1
                add("tmeasure", "t" + fam, sym, None, a, b, w, h, cs, profile, block=fam_blocks[fam][n % len(fam_blocks[fam])])
        add("tmeasure", "t" + fam, sym, None, "far16", "compact", 264, 70, "luv", 0, block=fam_blocks[fam][0])
    # 6. the plane-to-plane measures
    for fam in ms.FAMILIES:
        sym = "lumahip_planes_%s_frames_device" % fam
        for i, (a, b) in enumerate([("far16", "compact"), ("compact", "far16"), ("far16", "far16"), ("far16", "farodd"), ("wide", "wideodd")]):
            for (w, h, cs, profile) in _variants(i)[:2]:          # (no quantizer in these calls: the two Lu'v' variants)
                n += 1
                add("pmeasure", "p" + fam, sym, None, a, b, w, h, "luv", profile, block=fam_blocks[fam][n % len(fam_blocks[fam])])
        add("pmeasure", "p" + fam, sym, None, "far16", "compact", 264, 70, "luv", 0, block=fam_blocks[fam][0])
    # 7. the light level
    for i, form in enumerate(FORMS):
        sym = "lumahip_light_level_frames_device" + SUFFIX[form]
        for (w, h, cs, profile) in _variants(i)[:2]:              # (neither a quantizer nor planes: the two sizes)
            add("light", "light", sym, form, "planar3" if form.startswith("planar") else "far", None, w, h, "luv", 2)
    for i, a in enumerate(PLANE_KINDS):
        for (w, h, cs, profile) in _variants(i):
            add("light", "plight", "lumahip_planes_light_level_frames_device", None, a, None, w, h, cs, profile)
    add("light", "plight", "lumahip_planes_light_level_frames_device", None, "far16", None, 264, 70, "luv", 0)
    # 8. the stand-alone transform and the generator
    for (w, h) in SIZES:
        for cs in ("luv", "ycc"):
            add("frames", "transform", "lumahip_transform_color_space_device", None, "far", None, w, h, cs, 2)
        add("frames", "synth", "lumahip_synth_frames_device", None, "far", None, w, h, "luv", 2)
    # 10. launch shapes: one row per entry point again, as two workgroups of one wave and with 1024 threads asked for
    seen = set()
    for r in list(rows):
        if r.symbol in seen or r.group == "frames":
            continue
        seen.add(r.symbol)
        for shape in ("two", "1024"):
            rows.append(r._replace(id=r.id + "-" + shape, shape=shape))
    return rows


# ---- the inputs of a row and what the oracle (numpy for the words) makes of them
def tight(frames, w, h, profile):
    """frames of three (rows, >= row bytes) planes without their padding"""
    return [[np.ascontiguousarray(np.asarray(fr[p])[:plane_rows(w, h, profile, p)[0], :plane_rows(w, h, profile, p)[1]]) for p in range(3)]
            for fr in frames]


def oracle_encode(o, cfg, frames, profile, sc=1.0):
    """the oracle's tight planes of (nf, 3, h, w) float32 frames"""
    _, _, h, w = frames.shape
    return tight([fk.oracle(o, cfg).encode(np.array(fr, dtype=np.float32, copy=True), sc, profile)[0] for fr in frames], w, h, profile)


def oracle_decode(o, cfg, planes, profile, w, h, sc=1.0):
    """the oracle's (nf, 3, h, w) floats of frames of tight planes"""
    st = [plane_rows(w, h, profile, p)[1] for p in range(3)]
    return np.stack([fk.oracle(o, cfg).decode(fr, st, w, h, sc, profile) for fr in planes])


def code_planes(cfg, profile, w, h, nf):
    """nf distinct frames of tight code planes: plane_kernels.source_planes' three, and for the rotating decode a fourth, frame 0 with
    its rows rolled by one"""
    s = [list(fr) for fr in pk.source_planes(cfg, profile, w, h)]
    if nf == 1:
        return s[1:2]
    return s[:nf] if nf <= len(s) else s + [[np.roll(p, 1, axis=0) for p in s[0]]]


def halves_of(row):
    return row.form in ("f16", "planar_f16")


Inputs = collections.namedtuple("Inputs", "frames planes_a planes_b")


def true_inputs(o, row):
    """what the call of a row reads: float frames ((nf, 3, h, w) float32; for the binary16 forms values that are halves), the planes of its
    first plane operand, and -- the measuring calls -- of its second.  The given planes of a measuring row are the expected planes
    perturbed (measuring.given_from), so they depend on the true inputs alone"""
    w, h, nf, cfg = row.w, row.h, row.nf, cfg_of(row.cs, row.profile)
    e = row.entry
    if e == "encode":
        return Inputs(_float_frames(row), None, None)
    if e in ("decode", "transcode", "half", "plight"):
        return Inputs(None, code_planes(cfg, row.profile, w, h, nf), None)
    if e == "display":
        rng = np.random.default_rng([w, h, row.profile, row.block, nf])
        return Inputs(None, oracle_encode(o, cfg, display_frames(rng, nf, w, h, *DISPLAY_SETS[row.block][2:], *DISPLAY_SETS[row.block][:2]), row.profile), None)
    if e in ms.FAMILIES:
        fr = _float_frames(row)
        return Inputs(fr, None, _given(row, oracle_encode(o, cfg, fr, row.profile)))
    if e in ("tdistortion", "tdistortion_map", "tmoments_map"):
        s = code_planes(cfg, row.profile, w, h, nf)
        return Inputs(None, s, _given(row, oracle_encode(o, cfg, oracle_decode(o, cfg, s, row.profile, w, h), row.profile)))
    if e in ("pdistortion", "pdistortion_map", "pmoments_map"):
        a, b, _ = two_sets(case_rng(row.profile, w, h), w, h, row.profile)
        a, b = tight(a, w, h, row.profile), tight(b, w, h, row.profile)
        return Inputs(None, a[1:2], b[1:2]) if nf == 1 else Inputs(None, a, b)
    if e == "light":
        return Inputs(ll.frames(w, h, halves_of(row))[:nf], None, None)
    if e == "transform":
        return Inputs(fk.frames(w, h, nf), None, None)
    if e == "synth":
        return Inputs(None, None, None)
    raise ValueError(e)


def _float_frames(row):
    fr = fk.frames(row.w, row.h, 3, halves_of(row))
    fr = fr[1:2] if row.nf == 1 else fr
    return widen_halves(fr) if halves_of(row) else fr


def _given(row, e):
    fam = family_of(row)
    rng = np.random.default_rng([ms.FAMILIES.index(fam), row.w, row.h, row.profile, row.block or 0, len(row.symbol)])
    return ms.given_from(rng, fam, e, row.w, row.h, row.profile, row.block)[0]


def family_of(row):
    return row.entry if row.entry in ms.FAMILIES else row.entry[1:]


def expectation(o, row, inp):
    """what the call of a row must deliver for these inputs: frames of tight planes (encode, transcode, half), (nf, 3, h, w) floats
    (decode, transform; the binary16 forms: halves as uint16) or words"""
    w, h, cfg, e = row.w, row.h, cfg_of(row.cs, row.profile), row.entry
    if e == "encode":
        return oracle_encode(o, cfg, inp.frames, row.profile)
    if e == "decode":
        d = oracle_decode(o, cfg, inp.planes_a, row.profile, w, h)
        return float_to_half_np(d) if halves_of(row) else d
    if e == "display":
        return np.stack([display_bytes(t) for t in display_ts(o, row, inp)])
    if e == "transcode":
        return oracle_encode(o, cfg, oracle_decode(o, cfg, inp.planes_a, row.profile, w, h), row.profile)
    if e == "half":
        return oracle_encode(o, cfg, th.box(oracle_decode(o, cfg, inp.planes_a, row.profile, w, h)), row.profile)
    if e in ms.FAMILIES:
        return ms.words_of(e, oracle_encode(o, cfg, inp.frames, row.profile), inp.planes_b, w, h, row.profile, row.block)
    if e in ("tdistortion", "tdistortion_map", "tmoments_map"):
        enc = oracle_encode(o, cfg, oracle_decode(o, cfg, inp.planes_a, row.profile, w, h), row.profile)
        return ms.words_of(e[1:], enc, inp.planes_b, w, h, row.profile, row.block)
    if e in ("pdistortion", "pdistortion_map", "pmoments_map"):
        return ms.words_of(e[1:], inp.planes_a, inp.planes_b, w, h, row.profile, row.block)
    if e == "light":
        return ll.model_frames(inp.frames, LIGHT_SCALE)
    if e == "plight":
        return ll.model_frames(oracle_decode(o, cfg, inp.planes_a, row.profile, w, h), LIGHT_SCALE)
    if e == "transform":
        return np.stack([fk.oracle(o, cfg).transform(np.array(fr, dtype=np.float32, copy=True), True, 1.0) for fr in inp.frames])
    if e == "synth":
        return np.stack([o.synth_frame(w, h, frame=f) for f in range(row.nf)])
    raise ValueError(e)


def display_ts(o, row, inp):
    """per frame the (h, w, 3) float64 t of tests/support/display.py display_t for the oracle's decode of the planes"""
    do_tmo, ldr_sim, exposure, gamma = DISPLAY_SETS[row.block]
    d = oracle_decode(o, cfg_of(row.cs, row.profile), inp.planes_a, row.profile, row.w, row.h)
    return [display_t(fr, exposure, gamma, do_tmo, ldr_sim) for fr in d]


def same(a, b):
    """two expectations are the same, bit for bit"""
    if isinstance(a, list):
        return all(np.array_equal(x, y) for fa, fb in zip(a, b) for x, y in zip(fa, fb))
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float32:
        return same_bits(a, b)
    return bool(np.array_equal(a, b))


def operands(row):
    """[(which, role, kind)] of a row's far operands: which = "frames" / "planes_a" / "planes_b", role = "in" / "out" """
    e, out = row.entry, []
    if e == "encode":
        ops = [("frames", "in", row.a), ("planes_a", "out", row.b)]
    elif e == "decode":
        ops = [("planes_a", "in", row.a), ("frames", "out", row.b)]
    elif e == "display":
        ops = [("planes_a", "in", row.a), ("rgba", "out", row.b)]
    elif e in ("transcode", "half"):
        ops = [("planes_a", "in", row.a), ("planes_b", "out", row.b)]
    elif e in ms.FAMILIES:
        ops = [("frames", "in", row.a), ("planes_b", "in", row.b)]
    elif e in ("light", "transform"):
        ops = [("frames", "in", row.a)] + ([("frames", "out", row.a)] if e == "transform" else [])
    elif e == "synth":
        ops = [("frames", "out", row.a)]
    elif e == "plight":
        ops = [("planes_a", "in", row.a)]
    else:
        ops = [("planes_a", "in", row.a), ("planes_b", "in", row.b)]
    for which, role, kind in ops:
        if kind not in (None, "compact"):
            out.append((which, role, kind))
    return out


def dims_of(row, which):
    """(w, h) of an operand: the target of the half-resolution transcode is half the size"""
    return (row.w // 2, row.h // 2) if (row.entry == "half" and which == "planes_b") else (row.w, row.h)


def live_bytes(row):
    """device memory the far operands of a row hold at once"""
    total = 0
    for which, kind in sorted(set((which, kind) for which, _, kind in operands(row))):     # (the transform's frames are read and written)
        w, h = dims_of(row, which)
        esz = 2 if halves_of(row) else 4
        if kind == "fardisp":
            total += disp_layout(w, h, row.nf).alloc
        elif kind == "planar3":
            total += 3 * (PLANAR3_BYTES + LEAD + row.nf * (w * h + PAD) * esz + SLACK)
        elif kind in FRAME_KINDS:
            fl = frames_layout(kind, w, h, row.nf, esz)
            total += fl.alloc * esz
        else:
            total += planes_layout(kind, w, h, row.profile, row.nf).alloc
    return total


# ---- the device buffers (torch is imported inside, so that importing this module needs no GPU)
def _dev():
    import torch
    return torch.device("cuda:0")


def count_not_sentinel(t):
    """bytes of a uint8 tensor that are not the sentinel, looked at in pieces of CHUNK"""
    import torch
    total = torch.zeros((), dtype=torch.int64, device=t.device)
    for a in range(0, t.numel(), CHUNK):
        total += torch.count_nonzero(t[a:a + CHUNK] != SENTINEL)
    return int(total)


def free_bytes():
    import torch
    torch.cuda.empty_cache()
    return torch.cuda.mem_get_info()[0]


class _Far:
    """one device allocation of sentinel bytes and the 2-d views of its sample regions"""

    def _alloc(self, nbytes):
        import torch
        self.t = torch.full((nbytes,), SENTINEL, dtype=torch.uint8, device=_dev())

    def _views(self):
        raise NotImplementedError

    def samples(self):
        """the sample regions' bytes, gathered on the device: a list of uint8 numpy arrays"""
        return [v.contiguous().cpu().numpy() for v in self._views()]

    def only_samples_written(self):
        """nothing but the sample regions left the sentinel: the count over the whole allocation is the count in the regions"""
        import torch
        inside = sum(int(torch.count_nonzero(v != SENTINEL)) for v in self._views())
        return count_not_sentinel(self.t) == inside

    def unchanged(self):
        """the whole allocation is as it was: the samples as they were put, the sentinel everywhere else"""
        return self.only_samples_written() and all(np.array_equal(a, b) for a, b in zip(self.samples(), self.put))


class FarFrames(_Far):
    """frames on the device as tests/support/device.py Frames presents them -- .ptr, .fs, .nf, .w, .h, .n, .t, .host -- in the "far"
    layout (or, lead and fs given, any other): frame f at .ptr + f * fs elements, .ptr `lead` elements into the allocation"""

    def __init__(self, frames, dtype=np.float32, fs=None, lead=LEAD):
        import torch
        nf, _, h, w = frames.shape
        self.nf, self.w, self.h, self.n, self.dtype = nf, w, h, w * h, np.dtype(dtype)
        fl = frames_layout("far", w, h, nf, self.dtype.itemsize)
        self.fs, self.lead, self.esz = fl.fs if fs is None else fs, lead, self.dtype.itemsize
        self.host = np.empty(0, dtype=dtype)     # (device.py _frame_fed asks for the element size through it)
        self._alloc((lead + (nf - 1) * self.fs + 3 * self.n + SLACK) * self.esz)
        self.put = [np.ascontiguousarray(frames[f].astype(dtype)).view(np.uint8).ravel() for f in range(nf)]
        for f, v in enumerate(self._views()):
            v.copy_(torch.from_numpy(self.put[f]).to(_dev()))

    def _views(self):
        n = 3 * self.n * self.esz
        return [self.t[(self.lead + f * self.fs) * self.esz:][:n] for f in range(self.nf)]

    @property
    def ptr(self):
        return self.t.data_ptr() + self.lead * self.esz


class FarFloatOut(_Far):
    """the buffer a call writes nf frames of floats (or halves) into, as device.py FloatOut presents it, in the "far" layout or, with
    `rot`, the rotating one: frame f at .rot[f % 3] + (f // 3) * fs"""

    def __init__(self, nf, w, h, dtype=np.float32, fs=None, lead=LEAD, rot=False):
        self.nf, self.w, self.h, self.n, self.n3, self.dtype = nf, w, h, w * h, 3 * w * h, np.dtype(dtype)
        self.esz = self.dtype.itemsize
        self.fl = frames_layout("rot" if rot else "far", w, h, nf, self.esz)
        self.fs, self.lead = self.fl.fs if fs is None else fs, lead
        if fs is not None or lead != LEAD:
            self.fl = self.fl._replace(fs=self.fs, lead=lead, bases=(lead,), alloc=lead + (nf - 1) * self.fs + self.n3 + SLACK)
        self._alloc(self.fl.alloc * self.esz)
        self.put = [np.full(self.n3 * self.esz, SENTINEL, dtype=np.uint8)] * nf

    def _views(self):
        return [self.t[frame_offset(self.fl, f) * self.esz:][:self.n3 * self.esz] for f in range(self.nf)]

    @property
    def ptr(self):
        return self.t.data_ptr() + self.lead * self.esz

    @property
    def rot(self):
        return [self.t.data_ptr() + b * self.esz for b in self.fl.bases]

    def frames(self):
        """(nf, 3, h, w) of dtype: the sample regions, read back"""
        return np.stack([a.view(self.dtype).reshape(3, self.h, self.w) for a in self.samples()])


class FarPlanar(_Far):
    """layout "planar3": colour plane c of frame f at .plane_ptrs[c] + f * fs elements, fs = w h + PAD, the three colour planes in three
    allocations of PLANAR3_BYTES and more each, LEAD bytes into theirs.  frames: what to put (an input), or None (an output)"""

    def __init__(self, frames, nf, w, h, dtype=np.float32):
        import torch
        self.nf, self.w, self.h, self.n, self.dtype = nf, w, h, w * h, np.dtype(dtype)
        self.esz, self.fs, self.lead = self.dtype.itemsize, w * h + PAD, LEAD
        self.ts = [torch.full((PLANAR3_BYTES + LEAD + nf * self.fs * self.esz + SLACK,), SENTINEL, dtype=torch.uint8, device=_dev()) for _ in range(3)]
        nb = self.n * self.esz
        if frames is None:
            self.put = [np.full(nb, SENTINEL, dtype=np.uint8)] * (3 * nf)
        else:
            self.put = [np.ascontiguousarray(frames[f][c].astype(dtype)).view(np.uint8).ravel() for c in range(3) for f in range(nf)]
            for v, a in zip(self._views(), self.put):
                v.copy_(torch.from_numpy(a).to(_dev()))

    def _views(self):
        nb = self.n * self.esz
        return [self.ts[c][LEAD + f * self.fs * self.esz:][:nb] for c in range(3) for f in range(self.nf)]

    @property
    def plane_ptrs(self):
        return [t.data_ptr() + LEAD for t in self.ts]

    def only_samples_written(self):
        import torch
        inside = sum(int(torch.count_nonzero(v != SENTINEL)) for v in self._views())
        return sum(count_not_sentinel(t) for t in self.ts) == inside

    def frames(self):
        s = self.samples()
        return np.stack([np.stack([s[c * self.nf + f].view(self.dtype).reshape(self.h, self.w) for c in range(3)]) for f in range(self.nf)])


class FarDisplay(_Far):
    """the RGBA output of the display decode in disp_layout: .ptr, .st (the pitch), .fs (the frame stride), both in bytes"""

    def __init__(self, nf, w, h):
        self.nf, self.w, self.h = nf, w, h
        self.dl = disp_layout(w, h, nf)
        self.st, self.fs = self.dl.st, self.dl.dfs
        self._alloc(self.dl.alloc)
        self.put = [np.full((h, 4 * w), SENTINEL, dtype=np.uint8)] * nf

    def _views(self):
        return [self.t.as_strided((self.h, 4 * self.w), (self.st, 1), disp_offset(self.dl, f, 0)) for f in range(self.nf)]

    @property
    def ptr(self):
        return self.t.data_ptr() + self.dl.lead

    def images(self):
        return [a.reshape(self.h, self.w, 4) for a in self.samples()]


class FarPlanes(_Far):
    """nf frames of code planes in one sparse allocation, as device.py Planes presents a set -- .ptrs, .st, .pfs, .profile, .nf, .w, .h:
    plane p of frame f at .ptrs[p] + f * pfs[p], rows st[p] bytes apart.  kind: one of PLANE_KINDS; strides / pfs / lead override its
    numbers.  fill_frames: frames of three (rows, >= row bytes) planes to put (an input), or None (an output)"""

    def __init__(self, L, w, h, profile, nf, fill_frames=None, strides=None, pfs=None, lead=LEAD, kind="far16"):
        import torch
        self.w, self.h, self.profile, self.nf, self.kind = w, h, profile, nf, kind
        pl = planes_layout(kind, w, h, profile, nf)
        if strides is not None or pfs is not None or lead != LEAD:
            st = tuple(strides) if strides is not None else pl.st
            pf = tuple(pfs) if pfs is not None else pl.pfs
            off = tuple(o - LEAD + lead for o in pl.off)
            end = max(off[p] + (nf - 1) * pf[p] + (pl.rows[p] - 1) * st[p] + pl.rb[p] for p in range(3))
            pl = pl._replace(st=st, pfs=pf, lead=lead, off=off, alloc=end + SLACK)
        self.pl, self.st, self.pfs = pl, pl.st, list(pl.pfs)
        self._alloc(pl.alloc)
        if fill_frames is None:
            self.put = [np.full((pl.rows[p], pl.rb[p]), SENTINEL, dtype=np.uint8) for _ in range(nf) for p in range(3)]
        else:
            self.put = [np.array(np.asarray(fill_frames[f][p])[:pl.rows[p], :pl.rb[p]], order="C") for f in range(nf) for p in range(3)]
            for v, a in zip(self._views(), self.put):
                v.copy_(torch.from_numpy(a).to(_dev()))

    def _views(self):
        pl = self.pl
        return [self.t.as_strided((pl.rows[p], pl.rb[p]), (pl.st[p], 1), pl.off[p] + f * pl.pfs[p]) for f in range(self.nf) for p in range(3)]

    @property
    def ptrs(self):
        return [self.t.data_ptr() + o for o in self.pl.off]

    def host_frames(self):
        """the frames as lists of three tight (rows, row bytes) arrays: the rows' bytes only, gathered on the device"""
        s = self.samples()
        return [s[3 * f:3 * f + 3] for f in range(self.nf)]

    def frame(self, f):
        return self.host_frames()[f]
