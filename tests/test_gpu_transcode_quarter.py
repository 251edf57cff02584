"""Quarter-resolution transcode (include/lumahip_rungs.h lumahip_transcode_quarter_frames_device / lumahip_transcode_quarter_frame_host):
source planes of w x h under the source quantizer -> planes of (w/4) x (h/4) under the context's quantizer, the 2x2 box in linear
light twice on floats in between, one launch -- needs an MI355X.

Every comparison of planes is exact equality with the model of tests/support/transcode_quarter.py: the ORACLE's decode of the source
planes, numpy's float32 box(box(d)), the ORACLE's encode of that under the target configuration.  Nothing the library wrote enters
it.  Every launch has three distinct frames of seeded codes; before a call the destination holds the sentinel in a layout wider than
its rows, and every byte that is no sample must survive.  tests/test_transcode_quarter_host.py derives the set of kernels from the
matrix and holds the inputs of every row to the conditions that let it fail.

k_transcode_quarter<CSD, SUBD, CSE, SUBE, VW, LM> (lumahip_pick.hpp pick_planes<TransQuarterFamily, .>), 48 kernels:
  test_quarter_matrix              every kernel, statistics on every other row (min and max bit for bit, the sum within 1e-4)
  test_every_quarter_kernel_in_other_launch_shapes   1024 threads asked for (the plan's clamp to lh::transquarter_threads_bound), two
                                   workgroups of one wave, blocks_per_cu 1, one workgroup
  test_quarter_plane_sets_off_their_alignment        odd bases / strides / frame strides on either side; one set half a unit off
  test_frame_gaps_sections_and_the_host_form
  test_both_quantizers_are_left_alone
  test_refusals_launch_nothing     every refusal of the header with its message, the destination untouched
  test_two_half_calls_are_another_picture            the header's statement: chained half-resolution calls differ, the quarter call is the model"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.support import frame_kernels as fk  # noqa: E402
from tests.support import measuring as ms  # noqa: E402
from tests.support import plane_kernels as pk  # noqa: E402
from tests.support import transcode_quarter as tq  # noqa: E402
from tests.support.device import L, Planes, ctx, fused, on_device, stats_buf  # noqa: E402,F401  (L is the module fixture)
from tests.support.host import GAP, SENTINEL, plane_rows, same_rows  # noqa: E402

NF = tq.NF
ROWS = tq.quarter_matrix()
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


def quarter_call(c, src, src_sc, dst, dst_sc, stats=None):
    c.transcode_quarter_frames_device(src.ptrs, src.st, src.pfs, src.profile, src_sc, src.nf, src.w, src.h,
                                      dst.ptrs, dst.st, dst.pfs, dst.profile, dst_sc, stats.data_ptr() if stats is not None else None)


def quartered(L, c, src, src_sc, dp, dst_sc, stats=False, lay=None):
    """one lumahip_transcode_quarter_frames_device launch into sentinel-filled planes of (w/4) x (h/4), in the wide layout or in (row
    strides, gap, base): (the Planes, their host buffers, the per-frame {sum, min, max} or None)"""
    import torch
    tw, t_h = src.w // 4, src.h // 4
    st, gap, base = lay if lay is not None else (fk.wide_layout(tw, t_h, dp), GAP, 0)
    dst = Planes(L, tw, t_h, dp, src.nf, strides=st, gap=gap, base=base)
    sd = stats_buf(src.nf) if stats else None
    quarter_call(c, src, src_sc, dst, dst_sc, sd)
    torch.cuda.synchronize()
    return dst, dst.host(), (sd.cpu().numpy().reshape(src.nf, 3) if stats else None)


def written_planes_asserted(dst, bufs, e, tag):
    """every sample the model's, every other byte of the destination the sentinel"""
    problem = fk.planes_problem(bufs, e, dst.w, dst.h, dst.profile, dst.st, dst.gap, dst.base)
    assert problem is None, tag + (problem,)


# ---- 1. the matrix
@pytest.mark.parametrize("row", [pytest.param(r, id=r.id) for r in ROWS])
def test_quarter_matrix(L, oracle_mod, row):
    c = context(L, row.dcfg, row.scfg)
    front_end_asserted(c, row)
    ex = tq.expected_of(oracle_mod, row)
    src = laid_out(L, ex.s, row.w, row.h, row.sp)
    dst, bufs, got = quartered(L, c, src, row.src_sc, row.dp, row.dst_sc, row.stats)
    written_planes_asserted(dst, bufs, ex.e, (row.id,))
    if row.stats:
        for f in range(NF):
            want = fk.expected_stats(oracle_mod, row.dcfg, ex.m[f], row.dst_sc)
            print("%s frame %d: {sum, min, max} %r, numpy's on the model's frame %r" % (row.id, f, tuple(got[f]), want))
            problem = fk.stats_problem(got[f], want)
            assert problem is None, (row.id, f, problem)
    assert src.unchanged(), (row.id, "a source plane changed")


# ---- 2. the launch bounds and the persistent loop
SHAPES = {"1024_threads": (("block", 1024),), "two_workgroups_of_64": (("grid_enc", 2), ("block", 64)), "one_block_per_cu": (("blocks_per_cu", 1),),
          "one_workgroup": (("grid_enc", 1),)}
KERNEL_GROUPS = [pytest.param(csd, cse, sp, dp, w, h, id="%s-%s-p%d-p%d-%dx%d" % (fk.SPACES[csd][0], fk.SPACES[cse][0], sp, dp, w, h))
                 for (csd, cse) in pk.PAIRS for sp in tq.PROFILES for dp in tq.PROFILES for (w, h) in tq.ORDER_SIZES]


@pytest.mark.parametrize("csd,cse,sp,dp,w,h", KERNEL_GROUPS)
def test_every_quarter_kernel_in_other_launch_shapes(L, oracle_mod, csd, cse, sp, dp, w, h):
    """k_transcode_quarter<CSD, SUBD, CSE, SUBE, VW, every LM of the target> asked to run with 1024 threads -- transcode_plan clamps the
    launch to lh::transquarter_threads_bound, and a kernel compiled for fewer threads than its plan allows fails to launch --, as two
    workgroups of one wave (the persistent loop over the target's tiles, the frame change inside it, the last prefetch off the end), with
    one workgroup per CU and as one workgroup.  The planes of the default launch and the model's, all"""
    rows = [r for r in ROWS if (r.csd, r.cse, r.sp, r.dp, r.w, r.h) == (csd, cse, sp, dp, w, h) and not r.eight and
            r.src_sc == pk.scalings(csd, cse, r.lm)[-1][0]]
    assert sorted(tq.kernel_of(r)[5] for r in rows) == [lm for (cs, lm) in pk.TARGETS if cs == cse]
    for row in rows:
        ex = tq.expected_of(oracle_mod, row)
        src = laid_out(L, ex.s, w, h, sp)
        _, default, _ = quartered(L, context(L, row.dcfg, row.scfg), src, row.src_sc, dp, row.dst_sc)
        for shape, tunes in SHAPES.items():
            c = context(L, row.dcfg, row.scfg, tunes)
            front_end_asserted(c, row)
            dst, bufs, _ = quartered(L, c, src, row.src_sc, dp, row.dst_sc)
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
def test_quarter_plane_sets_off_their_alignment(L, oracle_mod, csd, cse, sp, dp, kind):
    """odd: every plane of the set one byte into its buffer, odd row strides, odd frame strides, at 528x144 (units of four samples) and
    536x152 (two), by 8- and 16-bit samples.  half: 528x144, the set half a four-sample unit off, strides multiples of 8 -- the plan
    must take two pixels per thread and keep the vector accesses.  The planes of the aligned call and the model's"""
    lm = LAYOUT_PAIRS[(csd, cse)]
    scfg, dcfg = pk.side_cfg(csd, 3, sp), pk.side_cfg(cse, lm, dp)
    src_sc, dst_sc = pk.scalings(csd, cse, lm)[-1]
    c = context(L, dcfg, scfg)
    which, how = kind.split("-")
    for (w, h) in (tq.ORDER_SIZES if how == "odd" else tq.ORDER_SIZES[:1]):
        tw, t_h = w // 4, h // 4
        ex = tq.expected(oracle_mod, scfg, dcfg, sp, dp, w, h, src_sc, dst_sc)
        slay = layout_of(how, w, h, sp) if which in ("src", "both") else None
        tlay = layout_of(how, tw, t_h, dp) if which in ("tgt", "both") else None
        src, plain = laid_out(L, ex.s, w, h, sp, slay), laid_out(L, ex.s, w, h, sp)
        tag = (fk.SPACES[csd][0], fk.SPACES[cse][0], sp, dp, kind, w, h)
        if slay is not None:
            parities_asserted(how, src, tag + ("source",))
        if tlay is not None:
            parities_asserted(how, Planes(L, tw, t_h, dp, NF, strides=tlay[0], gap=tlay[1], base=tlay[2]), tag + ("destination",))
        dst, bufs, _ = quartered(L, c, src, src_sc, dp, dst_sc, lay=tlay)
        written_planes_asserted(dst, bufs, ex.e, tag)
        adst, abufs, _ = quartered(L, c, plain, src_sc, dp, dst_sc)
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
    for (w, h) in tq.ORDER_SIZES:
        tw, t_h = w // 4, h // 4
        tag = (fk.SPACES[csd][0], fk.SPACES[cse][0], w, h)
        ex = tq.expected(oracle_mod, scfg, dcfg, sp, dp, w, h, src_sc, dst_sc)
        # a gap between frames on both sides, another one per plane and side
        src = laid_out(L, ex.s, w, h, sp, (fk.wide_layout(w, h, sp), (208, 16, 80), 0))
        dst, bufs, _ = quartered(L, c, src, src_sc, dp, dst_sc, lay=(fk.wide_layout(tw, t_h, dp), (32, 400, 96), 0))
        assert [dst.pfs[p] - dst.size[p] for p in range(3)] == [32, 400, 96] and [src.pfs[p] - src.size[p] for p in range(3)] == [208, 16, 80], tag
        written_planes_asserted(dst, bufs, ex.e, tag + ("gaps",))
        # twice inside an unordered section
        import torch
        plain = laid_out(L, ex.s, w, h, sp)
        lanes = [Planes(L, tw, t_h, dp, NF, strides=fk.wide_layout(tw, t_h, dp)) for _ in range(2)]
        c.begin_unordered(2)
        for d in lanes:
            quarter_call(c, plain, src_sc, d, dst_sc)
        c.end_unordered()
        c.sync()
        torch.cuda.synchronize()
        for d in lanes:
            written_planes_asserted(d, d.host(), ex.e, tag + ("unordered section",))
        # the host form: frame 0, the library's own strides for the quarter-size planes
        sst = [plane_rows(w, h, sp, p)[1] for p in range(3)]
        hp, hst = c.transcode_quarter_frame(ex.s[0], sst, w, h, src_sc, sp, dst_sc, dp)
        assert tuple(hst) == tuple(L.plane_geometry(tw, t_h, dp)[2]), tag
        assert same_rows(hp, ex.e[0], tw, t_h, dp), tag + ("host form against the model",)
        assert same_rows(hp, dst.frame(bufs, 0), tw, t_h, dp), tag + ("host form against the device form",)
        assert src.unchanged() and plain.unchanged(), tag


# ---- 5. the quantizers
def test_both_quantizers_are_left_alone(L, oracle_mod):
    """the quantizer's description and the planes lumahip_transcode_frames_device writes -- which read both quantizers -- are what they
    were before the quarter-resolution calls, device and host form"""
    import torch
    scfg, dcfg = pk.side_cfg(fk.YCC, 3, 2), pk.side_cfg(fk.LUV, 3, 2)
    c = ctx(L, dcfg, scfg)
    w, h = tq.SIZES[0]
    ex = tq.expected(oracle_mod, scfg, dcfg, 2, 2, w, h, 20.0, 1.0)
    src = laid_out(L, ex.s, w, h, 2)

    def full():
        dst = Planes(L, w, h, 2, NF)
        fused(c, src, 20.0, dst, 1.0)
        torch.cuda.synchronize()
        return dst.host(), c.quantizer_info()

    before = full()
    dst, bufs, _ = quartered(L, c, src, 20.0, 2, 1.0, stats=True)
    written_planes_asserted(dst, bufs, ex.e, ("quantizers",))
    c.transcode_quarter_frame(ex.s[0], [plane_rows(w, h, 2, p)[1] for p in range(3)], w, h, 20.0, 2, 1.0, 2)
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

    def attempt(c, code, w=w, h=h, dst=None, src=None, says=None):
        src = src or Planes(L, 64, 32, 2, 2)
        dst = dst or Planes(L, 16, 8, 2, 2)
        with pytest.raises(LumaHipError) as e:
            c.transcode_quarter_frames_device(src.ptrs, src.st, src.pfs, 2, 1.0, 2, w, h, dst.ptrs, dst.st, dst.pfs, 2, 1.0)
        assert e.value.code == code, str(e.value)
        message = c.L.lumahip_last_error(c.h).decode()
        assert message != "" and (says is None or says in message), message
        torch.cuda.synchronize()
        assert dst.unchanged(), "an error return wrote to the destination"

    def works(c):
        src, dst = Planes(L, w, h, 2, 2), Planes(L, w // 4, h // 4, 2, 2)
        quarter_call(c, src, 1.0, dst, 1.0)
        torch.cuda.synchronize()
        assert not dst.unchanged() and dst.gaps_intact(dst.host())

    c = ctx(L, luv)
    attempt(c, ERR_STATE, says="source quantizer not set")   # no source quantizer
    c0 = ctx(L, luv, luv, quantizer=False)
    attempt(c0, ERR_STATE)                                   # no quantizer
    c.set_source_quantizer(*luv, lut(luv))
    works(c)
    # w or h not a multiple of 8: multiples of 4 (legal for the half call), even, odd; and the issue's 4x8, 12x8, 8x12
    for bad in ((60, 32), (68, 32), (64, 28), (64, 36), (62, 32), (4, 8), (12, 8), (8, 12)):
        attempt(c, ERR_ARG, w=bad[0], h=bad[1], src=Planes(L, 72, 40, 2, 2), dst=Planes(L, 18, 10, 2, 2),
                says="Invalid frame size %dx%d (quarter resolution: must be multiples of 8)" % bad)
    for bad in ((63, 32), (64, 31)):                         # (odd sizes are the geometry check's, as in every call)
        attempt(c, ERR_ARG, w=bad[0], h=bad[1], src=Planes(L, 72, 40, 2, 2), dst=Planes(L, 18, 10, 2, 2))
    works(c)
    attempt(c, ERR_ARG, src=Planes(L, 32, 16, 2, 2))         # the source is checked at w x h: planes that hold only (w/2) x (h/2)
    small = Planes(L, 8, 4, 2, 2)
    attempt(c, ERR_ARG, dst=small)                           # the destination at (w/4) x (h/4): strides too small
    tight = Planes(L, 16, 4, 2, 2)
    attempt(c, ERR_ARG, dst=tight)                           # ... frame strides too small
    fits = Planes(L, 16, 8, 2, 2, strides=[plane_rows(16, 8, 2, p)[1] for p in range(3)], gap=0)
    quarter_call(c, Planes(L, w, h, 2, 2), 1.0, fits, 1.0)   # ... while planes that hold exactly the quarter-size frames are taken
    torch.cuda.synchronize()
    assert not fits.unchanged()
    src = Planes(L, w, h, 2, 2)
    attempt(c, ERR_ARG, src=src, dst=src, says="overlap")    # a source plane shares bytes with a destination plane
    works(c)
    # nframes 0 with null pointers, as the transcode call treats it
    rc = c.L.lumahip_transcode_quarter_frames_device(c.h, None, None, None, 2, 1.0, 0, w, h, None, None, None, 2, 1.0, None)
    assert rc == ERR_ARG == c.L.lumahip_transcode_frames_device(c.h, None, None, None, 2, 1.0, 0, w, h, None, None, None, 2, 1.0, None)
    with pytest.raises(LumaHipError) as e:                   # a bad profile
        s, d = Planes(L, w, h, 2, 2), Planes(L, 16, 8, 2, 2)
        c.transcode_quarter_frames_device(s.ptrs, s.st, s.pfs, 4, 1.0, 2, w, h, d.ptrs, d.st, d.pfs, 2, 1.0)
    assert e.value.code == ERR_ARG and "source profile" in str(e.value)
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
        ctx(L, luv).transcode_quarter_frame(planes, (128, 64, 64), w, h)
    assert e.value.code == ERR_STATE
    with pytest.raises(LumaHipError) as e:
        c.transcode_quarter_frame(planes, (128, 64, 64), 60, 32)
    assert e.value.code == ERR_ARG and "quarter resolution: must be multiples of 8" in str(e.value)


# ---- 7. far plane sets
def test_far_plane_sets(L, oracle_mod):
    """source size 1040x24 (a plane set's planes lie fl.STAGGER bytes apart in its allocation: the largest that fits), three frames, kind far16 on both sides: plane frame strides of 2^31 + 16 (p + 1) bytes behind a lead of 2^31,
    so frame 2 of the source and of the destination lies beyond 2^32 bytes of its pointer -- the 64-bit frame and row offsets of the
    source units at (4 ux, 4 uy) and of the stores; two sparse allocations of 6 GiB live.  The planes are the model's and the near
    layout's, nothing but samples is written and the source is as it was"""
    import torch
    from tests.support import far_layouts as fl
    row = next(r for r in ROWS if (r.csd, r.cse, r.lm, r.sp, r.dp, r.w, r.h) == (fk.LUV, fk.LUV, 3, 2, 2) + tq.SIZES[1])
    ex = tq.expected_of(oracle_mod, row)
    c = context(L, row.dcfg, row.scfg)
    w, h, tw, t_h = row.w, row.h, row.w // 4, row.h // 4
    tag = ("far-" + row.id,)
    near_dst, near, _ = quartered(L, c, laid_out(L, ex.s, w, h, row.sp), row.src_sc, row.dp, row.dst_sc)
    written_planes_asserted(near_dst, near, ex.e, tag + ("near",))
    src = fl.FarPlanes(L, w, h, row.sp, NF, fill_frames=ex.s, kind="far16")
    dst = fl.FarPlanes(L, tw, t_h, row.dp, NF, kind="far16")
    assert src.t.numel() + dst.t.numel() <= 12 * fl.GIB + (1 << 20), tag
    for pl in (src, dst):
        assert all((NF - 1) * pl.pfs[p] >= 1 << 32 for p in range(3)), tag
        assert all(pl.pl.rows[p] * pl.pl.st[p] <= fl.STAGGER for p in range(3)), tag + ("the planes of a set overlap",)
    quarter_call(c, src, row.src_sc, dst, row.dst_sc)
    torch.cuda.synchronize()
    got = dst.host_frames()
    for f in range(NF):
        for p in range(3):
            want = np.asarray(ex.e[f][p])[:dst.pl.rows[p], :dst.pl.rb[p]]
            assert np.array_equal(got[f][p], want), tag + ("far", f, p, "against the model")
            assert np.array_equal(got[f][p], np.asarray(near_dst.frame(near, f)[p])[:dst.pl.rows[p], :dst.pl.rb[p]]), tag + ("far", f, p, "against the near layout")
    assert dst.only_samples_written(), tag + ("a byte that is no sample was written",)
    assert src.unchanged(), tag + ("a source plane changed",)


# ---- 8. the documented statement
def test_two_half_calls_are_another_picture(L, oracle_mod):
    """include/lumahip_rungs.h: the quarter call is NOT two half-resolution calls.  On the first Lu'v' -> Lu'v' row the intermediate
    rung is written under the target quantizer by one context, and a second context whose source quantizer is the target's halves it
    again: those planes differ from the quarter call's, which equal the model"""
    import torch
    row = next(r for r in ROWS if r.csd == fk.LUV and r.cse == fk.LUV)
    ex = tq.expected_of(oracle_mod, row)
    src = laid_out(L, ex.s, row.w, row.h, row.sp)
    dst, bufs, _ = quartered(L, context(L, row.dcfg, row.scfg), src, row.src_sc, row.dp, row.dst_sc)
    written_planes_asserted(dst, bufs, ex.e, (row.id, "the quarter call"))
    hw, hh, tw, t_h = row.w // 2, row.h // 2, row.w // 4, row.h // 4
    mid = Planes(L, hw, hh, row.dp, NF)
    c1 = context(L, row.dcfg, row.scfg)
    c1.transcode_half_frames_device(src.ptrs, src.st, src.pfs, src.profile, row.src_sc, NF, row.w, row.h,
                                    mid.ptrs, mid.st, mid.pfs, row.dp, row.dst_sc)
    torch.cuda.synchronize()
    c2 = context(L, row.dcfg, row.dcfg)          # the source quantizer set to the target's
    low = Planes(L, tw, t_h, row.dp, NF, strides=dst.st, gap=dst.gap, base=dst.base)
    c2.transcode_half_frames_device(mid.ptrs, mid.st, mid.pfs, row.dp, row.dst_sc, NF, hw, hh, low.ptrs, low.st, low.pfs, row.dp, row.dst_sc)
    torch.cuda.synchronize()
    chained = low.host()
    n = sum(int(np.count_nonzero(a != b)) for a, b in zip(chained, bufs))
    print("%s: %d bytes of the chained half calls' planes differ from the quarter call's" % (row.id, n))
    assert n >= 1, (row.id, "two half-resolution calls wrote the quarter call's planes")
