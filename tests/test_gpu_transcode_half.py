"""Half-resolution transcode (include/lumahip_compare.h lumahip_transcode_half_frames_device / lumahip_transcode_half_frame_host):
source planes of w x h under the source quantizer -> planes of (w/2) x (h/2) under the context's quantizer, the 2x2 box in linear
light in between, one launch -- needs an MI355X.

Every comparison of planes is exact equality with the model of tests/support/transcode_half.py: the ORACLE's decode of the source
planes, numpy's float32 ((a + b) + (c + d)) * 0.25, the ORACLE's encode of that under the target configuration.  Nothing the library
wrote enters it.  Every launch has three distinct frames of seeded codes (tests/support/plane_kernels.py source_planes); before a
call the destination holds the sentinel in a layout wider than its rows, and every byte that is no sample must survive.
tests/test_transcode_half_host.py derives the set of kernels from the matrix and holds the inputs of every row to the conditions
that let it fail (the top-left pixel, either pair alone and, Lu'v' -> Lu'v', two other orders of the sum change luma samples).

k_transcode_half<CSD, SUBD, CSE, SUBE, VW, LM> (lumahip_pick.hpp pick_planes<TransHalfFamily, .>), 48 kernels:
  test_half_matrix                 every kernel: both sources x targets LM 3 / 7 / 5 x profiles {2, 3}^2 x source sizes 264x72 (VW 4,
                                   several tile rows), 520x12 (VW 4, target 260 wide: past one tile column), 268x76 (target 134 wide:
                                   VW 2, past one tile column), 8x4 (one unit); a YCbCr source at preScaling 1, 20 and 3e5; the 8-bit
                                   profile pairs under 8-bit tables; on every other row the statistics against numpy on the model's frames
                                   (min and max bit for bit, the sum within 1e-4: the launch adds in another order)
  test_every_half_kernel_in_other_launch_shapes   two workgroups of one wave (the persistent loop, the frame change, the prefetch running off
                                   the end) and 1024 threads asked for (the plan's clamp to lh::transhalf_threads_bound)
  test_half_plane_sets_off_their_alignment        every base, row stride and frame stride odd, source / destination / both; one set half a
                                   four-sample unit off (VW 2 with vector accesses)
  test_frame_gaps_sections_and_the_host_form      unequal gaps between frames on both sides; the call twice inside an unordered section; the
                                   host form equal to the device form
  test_both_quantizers_are_left_alone
  test_refusals_launch_nothing     every refusal of the header returns its code and leaves the destination untouched"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.support import frame_kernels as fk  # noqa: E402
from tests.support import measuring as ms  # noqa: E402
from tests.support import plane_kernels as pk  # noqa: E402
from tests.support import transcode_half as th  # noqa: E402
from tests.support.device import L, Planes, ctx, fused, on_device, stats_buf  # noqa: E402,F401  (L is the module fixture)
from tests.support.host import GAP, SENTINEL, plane_rows, same_rows  # noqa: E402

NF = th.NF
ROWS = th.half_matrix()
_ctx = {}


def context(L, dcfg, scfg, tunes=()):
    """a context on torch's stream per (target configuration, source configuration, tunes), made once"""
    key = (dcfg, scfg, tuple(tunes))
    if key not in _ctx:
        c = ctx(L, dcfg, scfg)
        for name, v in tunes:
            c.tune(name, v)
        _ctx[key] = c
    return _ctx[key]


def front_end_asserted(c, row):
    """what transcode_plan picks the kernel by: the target's search mode, and for a YCbCr target that the composite records exist"""
    if row.cse == fk.YCC:
        assert c.quantizer_info()["mode"] == 3 and c.half_table_info(row.dst_sc)["used"], (row.id, "no composite records")
    else:
        assert c.quantizer_info()["mode"] == row.lm, row.id


def laid_out(L, frames, w, h, profile, lay=None):
    """the frames on the device in the wide layout, or in (row strides, gap, base)"""
    st, gap, base = lay if lay is not None else (None, GAP, 0)
    return on_device(L, ms.HostPlanes(frames, w, h, profile, st, gap, base))


def half_call(c, src, src_sc, dst, dst_sc, stats=None):
    c.transcode_half_frames_device(src.ptrs, src.st, src.pfs, src.profile, src_sc, src.nf, src.w, src.h,
                                   dst.ptrs, dst.st, dst.pfs, dst.profile, dst_sc, stats.data_ptr() if stats is not None else None)


def halved(L, c, src, src_sc, dp, dst_sc, stats=False, lay=None):
    """one lumahip_transcode_half_frames_device launch into sentinel-filled planes of (w/2) x (h/2), in the wide layout or in (row
    strides, gap, base): (the Planes, their host buffers, the per-frame {sum, min, max} or None)"""
    import torch
    tw, t_h = src.w // 2, src.h // 2
    st, gap, base = lay if lay is not None else (fk.wide_layout(tw, t_h, dp), GAP, 0)
    dst = Planes(L, tw, t_h, dp, src.nf, strides=st, gap=gap, base=base)
    sd = stats_buf(src.nf) if stats else None
    half_call(c, src, src_sc, dst, dst_sc, sd)
    torch.cuda.synchronize()
    return dst, dst.host(), (sd.cpu().numpy().reshape(src.nf, 3) if stats else None)


def written_planes_asserted(dst, bufs, e, tag):
    """every sample the model's, every other byte of the destination the sentinel"""
    problem = fk.planes_problem(bufs, e, dst.w, dst.h, dst.profile, dst.st, dst.gap, dst.base)
    assert problem is None, tag + (problem,)


# ---- 1. the matrix
@pytest.mark.parametrize("row", [pytest.param(r, id=r.id) for r in ROWS])
def test_half_matrix(L, oracle_mod, row):
    c = context(L, row.dcfg, row.scfg)
    front_end_asserted(c, row)
    ex = th.expected_of(oracle_mod, row)
    src = laid_out(L, ex.s, row.w, row.h, row.sp)
    dst, bufs, got = halved(L, c, src, row.src_sc, row.dp, row.dst_sc, row.stats)
    written_planes_asserted(dst, bufs, ex.e, (row.id,))
    if row.stats:
        for f in range(NF):
            want = fk.expected_stats(oracle_mod, row.dcfg, ex.m[f], row.dst_sc)
            print("%s frame %d: {sum, min, max} %r, numpy's on the model's frame %r" % (row.id, f, tuple(got[f]), want))
            problem = fk.stats_problem(got[f], want)
            assert problem is None, (row.id, f, problem)
    assert src.unchanged(), (row.id, "a source plane changed")


# ---- 2. the launch bounds and the persistent loop
SHAPES = {"1024_threads": (("block", 1024),), "two_workgroups_of_64": (("grid_enc", 2), ("block", 64))}
KERNEL_GROUPS = [pytest.param(csd, cse, sp, dp, w, h, id="%s-%s-p%d-p%d-%dx%d" % (fk.SPACES[csd][0], fk.SPACES[cse][0], sp, dp, w, h))
                 for (csd, cse) in pk.PAIRS for sp in th.PROFILES for dp in th.PROFILES for (w, h) in th.ORDER_SIZES]


@pytest.mark.parametrize("csd,cse,sp,dp,w,h", KERNEL_GROUPS)
def test_every_half_kernel_in_other_launch_shapes(L, oracle_mod, csd, cse, sp, dp, w, h):
    """k_transcode_half<CSD, SUBD, CSE, SUBE, VW, every LM of the target> asked to run with 1024 threads -- transcode_plan clamps the
    launch to lh::transhalf_threads_bound, and a kernel compiled for fewer threads than its plan allows fails to launch -- and as two
    workgroups of one wave: the persistent loop over the target's tiles, the frame change inside it, the last prefetch off the end.
    The planes of the default launch and the model's, all three"""
    rows = [r for r in ROWS if (r.csd, r.cse, r.sp, r.dp, r.w, r.h) == (csd, cse, sp, dp, w, h) and not r.eight and
            r.src_sc == pk.scalings(csd, cse, r.lm)[-1][0]]
    assert sorted(th.kernel_of(r)[5] for r in rows) == [lm for (cs, lm) in pk.TARGETS if cs == cse]
    for row in rows:
        ex = th.expected_of(oracle_mod, row)
        src = laid_out(L, ex.s, w, h, sp)
        _, default, _ = halved(L, context(L, row.dcfg, row.scfg), src, row.src_sc, dp, row.dst_sc)
        for shape, tunes in SHAPES.items():
            c = context(L, row.dcfg, row.scfg, tunes)
            front_end_asserted(c, row)
            dst, bufs, _ = halved(L, c, src, row.src_sc, dp, row.dst_sc)
            written_planes_asserted(dst, bufs, ex.e, (row.id, shape))
            assert all(np.array_equal(a, b) for a, b in zip(bufs, default)), (row.id, shape, "the default launch")
        assert src.unchanged(), row.id


# ---- 3. layouts the vector loads and stores cannot take
LAYOUT_PAIRS = {(fk.LUV, fk.LUV): 3, (fk.LUV, fk.YCC): 5, (fk.YCC, fk.LUV): 7, (fk.YCC, fk.YCC): 5}      # one LM per colour-space pair
LAYOUT_PROFILES = [(2, 2), (3, 3), (0, 1), (1, 0)]
KINDS = ["src-odd", "tgt-odd", "both-odd", "src-half", "tgt-half"]


def layout_of(kind, w, h, profile):
    """(row strides, gaps, base) of a plane set of this kind"""
    if kind == "odd":
        return fk.odd_layout(w, h, profile) + (1,)
    st, base = ms.half_aligned_layout(w, h, profile)
    return st, GAP, base


def parities_asserted(kind, pl, tag):
    if kind == "odd":
        assert all(p % 2 == 1 for p in pl.ptrs) and all(s % 2 == 1 for s in pl.st) and all(s % 2 == 1 for s in pl.pfs), tag
    else:       # four samples: 8 bytes, or 4
        unit = 8 if pl.profile > 1 else 4
        assert all(p % unit == unit // 2 for p in pl.ptrs) and all(s % 8 == 0 for s in tuple(pl.st) + tuple(pl.pfs)), tag


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("sp,dp", LAYOUT_PROFILES)
@pytest.mark.parametrize("csd,cse", list(LAYOUT_PAIRS), ids=lambda cs: fk.SPACES[cs][0])
def test_half_plane_sets_off_their_alignment(L, oracle_mod, csd, cse, sp, dp, kind):
    """odd: every plane of the set one byte into its buffer, odd row strides, odd frame strides -- DecArgs::aligned = 0 for the planes
    read, EncArgs::aligned = 0 and the byte-wise stores for the planes written, at 264x72 (units of four samples) and 268x76 (two), by
    8- and 16-bit samples.  half: 264x72, the set half a four-sample unit off, strides multiples of 8 -- the plan must take two pixels
    per thread and keep the vector accesses.  The planes of the aligned call and the model's; on an odd destination every byte around
    the samples shows whether a store ran past a row's end"""
    lm = LAYOUT_PAIRS[(csd, cse)]
    scfg, dcfg = pk.side_cfg(csd, 3, sp), pk.side_cfg(cse, lm, dp)
    src_sc, dst_sc = pk.scalings(csd, cse, lm)[-1]
    c = context(L, dcfg, scfg)
    which, how = kind.split("-")
    for (w, h) in (th.ORDER_SIZES if how == "odd" else th.ORDER_SIZES[:1]):
        tw, t_h = w // 2, h // 2
        ex = th.expected(oracle_mod, scfg, dcfg, sp, dp, w, h, src_sc, dst_sc)
        slay = layout_of(how, w, h, sp) if which in ("src", "both") else None
        tlay = layout_of(how, tw, t_h, dp) if which in ("tgt", "both") else None
        src, plain = laid_out(L, ex.s, w, h, sp, slay), laid_out(L, ex.s, w, h, sp)
        tag = (fk.SPACES[csd][0], fk.SPACES[cse][0], sp, dp, kind, w, h)
        if slay is not None:
            parities_asserted(how, src, tag + ("source",))
        if tlay is not None:
            parities_asserted(how, Planes(L, tw, t_h, dp, NF, strides=tlay[0], gap=tlay[1], base=tlay[2]), tag + ("destination",))
        dst, bufs, _ = halved(L, c, src, src_sc, dp, dst_sc, lay=tlay)
        written_planes_asserted(dst, bufs, ex.e, tag)
        adst, abufs, _ = halved(L, c, plain, src_sc, dp, dst_sc)
        written_planes_asserted(adst, abufs, ex.e, tag + ("the aligned call",))
        assert src.unchanged() and plain.unchanged(), tag + ("a source plane changed",)


# ---- 4. frame strides, unordered sections, the host form
@pytest.mark.parametrize("csd,cse", list(LAYOUT_PAIRS), ids=lambda cs: fk.SPACES[cs][0])
def test_frame_gaps_sections_and_the_host_form(L, oracle_mod, csd, cse):
    lm = LAYOUT_PAIRS[(csd, cse)]
    sp, dp = 2, 3
    scfg, dcfg = pk.side_cfg(csd, 3, sp), pk.side_cfg(cse, lm, dp)
    src_sc, dst_sc = pk.scalings(csd, cse, lm)[-1]
    c = context(L, dcfg, scfg)
    for (w, h) in th.ORDER_SIZES:
        tw, t_h = w // 2, h // 2
        tag = (fk.SPACES[csd][0], fk.SPACES[cse][0], w, h)
        ex = th.expected(oracle_mod, scfg, dcfg, sp, dp, w, h, src_sc, dst_sc)
        # a gap between frames on both sides, another one per plane and side
        src = laid_out(L, ex.s, w, h, sp, (fk.wide_layout(w, h, sp), (208, 16, 80), 0))
        dst, bufs, _ = halved(L, c, src, src_sc, dp, dst_sc, lay=(fk.wide_layout(tw, t_h, dp), (32, 400, 96), 0))
        assert [dst.pfs[p] - dst.size[p] for p in range(3)] == [32, 400, 96] and [src.pfs[p] - src.size[p] for p in range(3)] == [208, 16, 80], tag
        written_planes_asserted(dst, bufs, ex.e, tag + ("gaps",))
        # twice inside an unordered section
        import torch
        plain = laid_out(L, ex.s, w, h, sp)
        lanes = [Planes(L, tw, t_h, dp, NF, strides=fk.wide_layout(tw, t_h, dp)) for _ in range(2)]
        c.begin_unordered(2)
        for d in lanes:
            half_call(c, plain, src_sc, d, dst_sc)
        c.end_unordered()
        c.sync()
        torch.cuda.synchronize()
        for d in lanes:
            written_planes_asserted(d, d.host(), ex.e, tag + ("unordered section",))
        # the host form: frame 0, the library's own strides for the half-size planes
        sst = [plane_rows(w, h, sp, p)[1] for p in range(3)]
        hp, hst = c.transcode_half_frame(ex.s[0], sst, w, h, src_sc, sp, dst_sc, dp)
        assert tuple(hst) == tuple(L.plane_geometry(tw, t_h, dp)[2]), tag
        assert same_rows(hp, ex.e[0], tw, t_h, dp), tag + ("host form against the model",)
        assert same_rows(hp, dst.frame(bufs, 0), tw, t_h, dp), tag + ("host form against the device form",)
        assert src.unchanged() and plain.unchanged(), tag


# ---- 5. the quantizers
def test_both_quantizers_are_left_alone(L, oracle_mod):
    """the quantizer's description and the planes lumahip_transcode_frames_device writes -- which read both quantizers -- are what they
    were before the half-resolution calls, device and host form"""
    import torch
    scfg, dcfg = pk.side_cfg(fk.YCC, 3, 2), pk.side_cfg(fk.LUV, 3, 2)
    c = ctx(L, dcfg, scfg)
    w, h = th.SIZES[0]
    ex = th.expected(oracle_mod, scfg, dcfg, 2, 2, w, h, 20.0, 1.0)
    src = laid_out(L, ex.s, w, h, 2)

    def full():
        dst = Planes(L, w, h, 2, NF)
        fused(c, src, 20.0, dst, 1.0)
        torch.cuda.synchronize()
        return dst.host(), c.quantizer_info()

    before = full()
    dst, bufs, _ = halved(L, c, src, 20.0, 2, 1.0, stats=True)
    written_planes_asserted(dst, bufs, ex.e, ("quantizers",))
    c.transcode_half_frame(ex.s[0], [plane_rows(w, h, 2, p)[1] for p in range(3)], w, h, 20.0, 2, 1.0, 2)
    after = full()
    assert after[1] == before[1]
    assert all(np.array_equal(a, b) for a, b in zip(before[0], after[0]))
    assert not all(np.all(b == SENTINEL) for b in after[0])


# ---- 6. refusals
def test_refusals_launch_nothing(L):
    import torch
    from lumahdrv_amd.capi import ERR_ARG, ERR_STATE, ERR_UNSUPPORTED, LumaHipError
    w, h = 64, 32
    luv = pk.side_cfg(fk.LUV, 3, 2)

    def lut(cfg):
        return L.build_lut(cfg[0], cfg[1], cfg[4], cfg[5])

    def attempt(c, code, w=w, h=h, dst=None, src=None):
        src = src or Planes(L, 64, 32, 2, 2)
        dst = dst or Planes(L, 32, 16, 2, 2)
        with pytest.raises(LumaHipError) as e:
            c.transcode_half_frames_device(src.ptrs, src.st, src.pfs, 2, 1.0, 2, w, h, dst.ptrs, dst.st, dst.pfs, 2, 1.0)
        assert e.value.code == code, str(e.value)
        assert c.L.lumahip_last_error(c.h).decode() != ""
        torch.cuda.synchronize()
        assert dst.unchanged(), "an error return wrote to the destination"

    def works(c):
        src, dst = Planes(L, w, h, 2, 2), Planes(L, w // 2, h // 2, 2, 2)
        half_call(c, src, 1.0, dst, 1.0)
        torch.cuda.synchronize()
        assert not dst.unchanged() and dst.gaps_intact(dst.host())

    c = ctx(L, luv)
    attempt(c, ERR_STATE)                                    # no source quantizer
    c0 = ctx(L, luv, luv, quantizer=False)
    attempt(c0, ERR_STATE)                                   # no quantizer
    c.set_source_quantizer(*luv, lut(luv))
    works(c)
    for bad in ((62, 32), (66, 32), (64, 30), (64, 34), (63, 32), (64, 31)):     # w or h not a multiple of 4: even, and odd
        attempt(c, ERR_ARG, w=bad[0], h=bad[1], src=Planes(L, 68, 36, 2, 2), dst=Planes(L, 34, 18, 2, 2))
    works(c)
    attempt(c, ERR_ARG, src=Planes(L, 32, 16, 2, 2))         # the source is checked at w x h: planes that hold only (w/2) x (h/2)
    small = Planes(L, 16, 8, 2, 2)
    attempt(c, ERR_ARG, dst=small)                           # the destination at (w/2) x (h/2): strides too small
    tight = Planes(L, 32, 8, 2, 2)
    attempt(c, ERR_ARG, dst=tight)                           # ... frame strides too small
    fits = Planes(L, 32, 16, 2, 2, strides=[plane_rows(32, 16, 2, p)[1] for p in range(3)], gap=0)
    half_call(c, Planes(L, w, h, 2, 2), 1.0, fits, 1.0)      # ... while planes that hold exactly the half-size frames are taken
    torch.cuda.synchronize()
    assert not fits.unchanged()
    src = Planes(L, w, h, 2, 2)
    attempt(c, ERR_ARG, src=src, dst=src)                    # a source plane shares bytes with a destination plane
    works(c)
    # nframes 0 with null pointers, as the transcode call treats it
    rc = c.L.lumahip_transcode_half_frames_device(c.h, None, None, None, 2, 1.0, 0, w, h, None, None, None, 2, 1.0, None)
    assert rc == ERR_ARG == c.L.lumahip_transcode_frames_device(c.h, None, None, None, 2, 1.0, 0, w, h, None, None, None, 2, 1.0, None)
    works(c)
    for cs in (1, 3):                                        # RGB / XYZ on either side
        bad = (1, 11, cs, 8, 1e4, 0.005)
        c.set_source_quantizer(*bad, lut(bad))
        attempt(c, ERR_UNSUPPORTED)
        c.set_source_quantizer(*luv, lut(luv))
        works(c)
        attempt(ctx(L, bad, luv), ERR_UNSUPPORTED)
    deep = (1, 14, 0, 8, 1e4, 0.005)                         # source bit depth 14
    c.set_source_quantizer(*deep, lut(deep))
    attempt(c, ERR_UNSUPPORTED)
    c.set_source_quantizer(*luv, lut(luv))
    works(c)
    c.tune("force_literal", 1)                               # literal-bisection target
    attempt(c, ERR_UNSUPPORTED)
    c.tune("force_literal", 0)
    works(c)
    big, y12 = (1, 13, 0, 8, 1e4, 0.005), (1, 12, 2, 12, 1000.0, 0.01)   # 136 KiB of records + a 12-bit YCbCr source: beyond 160 KiB
    c3 = ctx(L, big, y12)
    attempt(c3, ERR_UNSUPPORTED)
    c3.set_source_quantizer(*luv, lut(luv))                  # ... while PQ-11 Lu'v' beside the 13-bit target fits
    works(c3)
    planes = [np.zeros((32, 128), np.uint8), np.zeros((16, 64), np.uint8), np.zeros((16, 64), np.uint8)]
    with pytest.raises(LumaHipError) as e:                   # the host form refuses the same way
        ctx(L, luv).transcode_half_frame(planes, (128, 64, 64), w, h)
    assert e.value.code == ERR_STATE
    with pytest.raises(LumaHipError) as e:
        c.transcode_half_frame(planes, (128, 64, 64), 66, 32)
    assert e.value.code == ERR_ARG
