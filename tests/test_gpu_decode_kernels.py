"""The plain decode with its table in LDS, every instantiation the pickers can return from the device entry points, in other launch
shapes and on the layouts its loads and stores cannot take as vectors -- needs an MI355X.

Every comparison is bit for bit (two NaN are the same).  What the kernels are held to is the ORACLE's decode of every frame's planes
(tests/support/decode_kernels.py expected: Oracle.decode; for binary16 frames float_to_half_np of its floats), never what another call of
the library wrote.  Every launch has three distinct frames of seeded in-range codes -- four on the rotating rows, so that one of the three
buffers holds two --; the 264x70 frames carry 0, 1, maxVal - 1, maxVal, maxVal + 1, maxC, maxC + 1 and all ones in an 8x16 corner, the
258x6 frames in a 4x16 corner: a chroma code beyond maxC sends Lu'v' chroma (luv_chroma<false>), the YT tables' `bad` and RB's `redo` to
the complete functions, in the four- and the two-pixel kernels.  The rb rows at 264x70 decode picture-like planes in frames 0 and 2 and
unrelated codes in frame 1.  Before a call the output buffers hold the sentinel, with 4 elements in front of the first frame and 4
behind every frame (planar: every colour plane); dk.frames_problem names the first value that differs by frame, channel, row and column
and holds every byte outside the frames to the sentinel; the source planes and their gaps are compared with what they were.
tests/test_decode_kernels_host.py derives the set of kernels and shows that the inputs can fail a wrong kernel: the expected frames are
informative, the comparison rejects planted errors, and seven wrong kernels modelled with the oracle fail every row they apply to.

k_decode<CS, SUB, VW, GL = false, DISP = false, YT, RB, OUT16> (lumahip_pick.hpp pick_dec<false> / pick_dec_f16; dk.kernel_of restates the
choice of decode_impl and is asserted against what the row is meant to name before anything is compared; quantizer_info says that the
table is in LDS; rb_table_info "table_launches" is read around every launch: + 1 on an rb row, + 0 on every other):
  plain     test_decode_matrix[luv-* rgb-* xyz-* ycbcr-plain-*]   PQ-11 Lu'v', RGB, XYZ; PQ-10 YCbCr (maxLum 1000, colour depth 10) under
                                                                  "ycbcr_tables" 0
  YT        test_decode_matrix[ycbcr-yt-*]                        the same YCbCr under "ycbcr_rb_tables" 0
  YT, RB    test_decode_matrix[ycbcr-rb-*]                        under "ycbcr_rb_tables" 2: every wave gathers, the lag policy never decides
each by SUB (profiles 2 and 3), VW 4 at 64x32 (one tile) and 264x70 (several tiles both ways), VW 2 at 258x6 (a ragged last tile) and
6x4, float and binary16 frames ([*-f32-*], [*-f16-*]): 48 kernels.  preScaling 1 and 20 on every one (YCbCr: sc_mode 0 and 1, the two
copies of dec_process; the others: with and without div_ieee), and 3e5 -- sc_mode 2, the complete functions' IEEE division -- on one 258x6
row per YCbCr variant.  The sample size is a kernel argument: profiles 0 and 1 run on two rows per (colour space, variant, frame
type) under the 8-bit table.  The call form goes round -- packed, planar (three separate buffers), rotating (DecArgs::rot, readfirstlane
on the frame index); binary16: packed, planar -- so that each form meets every (colour space, variant) at both vector widths.
  other launch shapes   test_every_kernel_in_other_launch_shapes   all 48 again at 264x70 and 258x6 with 1024 threads asked for and as two
                        workgroups of one wave ("grid_dec" 2, "block" 64: the persistent loop, the prefetch running off the end, the frame
                        change inside it); the bytes of the expectation, not of the default launch

Layouts (plain YCbCr, YT, RB with float frames and all 24 OUT16 kernels: what tests/test_gpu_frame_kernels.py does not reach; profiles
0-3):
  every plane base, row stride and frame stride odd (64x32, 258x6)     test_source_planes_off_their_alignment[*-odd]     a.aligned = 0,
                                                                       units of four, two and one sample, 8- and 16-bit
  planes half a four-sample unit off, strides multiples of 8 (64x32)   test_source_planes_off_their_alignment[*-half]    VW 4 with aligned = 0
  frames two elements into a four-element unit (float: 8 bytes off 16, binary16: 4 off 8) / a frame stride of 3 w h + 2
                                                                       test_outputs_that_take_two_pixels_only   kernel_of says VW 2 at 64x32;
                                                                       the frames of the aligned launch and the oracle's
A context keeps its state: test_a_context_keeps_its_state -- the same planes twice and once inside begin_unordered(2) / end_unordered.

Left unrun: the tile-count thresholds of grid_for (`few_writers`, 6000 / 60000 tiles) lie far beyond these sizes.  They change the grid
size alone, and the rows with two workgroups cover correctness under any grid.  The four CS_PACK kernels are reached through
lumahip_unpack_frame_host only and stay with tests/test_gpu_frame_kernels.py test_pack_only_and_unpack_only."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.support import decode_kernels as dk  # noqa: E402
from tests.support import frame_kernels as fk  # noqa: E402
from tests.support import measuring as ms  # noqa: E402
from tests.support.device import FloatOut, L, ctx, dev, on_device  # noqa: E402,F401  (L is the module fixture)
from tests.support.host import GAP  # noqa: E402

ROWS = dk.decode_matrix()
_ctx = {}


def context(L, cfg, tunes=()):
    """a context on torch's stream per (configuration, tunes), made once"""
    key = (cfg, tuple(tunes))
    if key not in _ctx:
        c = ctx(L, cfg)
        for name, v in tunes:
            c.tune(name, v)
        _ctx[key] = c
    return _ctx[key]


class DeviceOut:
    """the buffers of a dk.OutLayout on the device, the sentinel in every byte"""

    def __init__(self, lay):
        import torch
        self.lay = lay
        self.t = [torch.from_numpy(b).to(dev()) for b in lay.blank()]

    def ptrs(self):
        return [t.data_ptr() + self.lay.base * self.lay.dtype.itemsize for t in self.t]

    def written(self):
        return dk.Written(self.lay, [t.cpu().numpy() for t in self.t])

    def frames(self):
        """(nf, 3, h, w) as the buffers hold them"""
        lay, bufs = self.written()
        return np.stack([np.stack([bufs[b].view(lay.dtype)[off:off + lay.n].reshape(lay.h, lay.w) for (b, off) in (lay.at(f, c) for c in range(3))])
                         for f in range(lay.nf)])


def laid_out(L, frames, w, h, profile, lay=None):
    """the source planes on the device in the wide layout, or in (row strides, gap, base)"""
    st, gap, base = lay if lay is not None else (None, GAP, 0)
    return on_device(L, ms.HostPlanes(frames, w, h, profile, st, gap, base))


def launch(c, pl, sc, out):
    """lumahip_decode_frames_device in the form and frame type of the output's layout"""
    import torch
    lay, p = out.lay, out.ptrs()
    args = (pl.ptrs, pl.st, pl.pfs, pl.nf, pl.w, pl.h, pl.profile, sc)
    if lay.form == "packed":
        (c.decode_frames_device_f16 if lay.out16 else c.decode_frames_device)(*args, p[0], lay.fs)
    elif lay.form == "planar":
        (c.decode_frames_device_planar_f16 if lay.out16 else c.decode_frames_device_planar)(*args, p, lay.fs)
    else:
        c.decode_frames_device_rotating(*args, p, lay.fs)
    torch.cuda.synchronize()


def named(row, vw):
    """the kernel a row is meant to name"""
    return (row.cs, row.profile in (0, 2), vw, row.cs == fk.YCC and row.variant != "plain", row.variant == "rb", row.out16)


def held(L, o, c, row, vw, lay=None, src_lay=None, tag=()):
    """one launch of the row's call held to the oracle: the kernel it names, the table launches it counts, every byte of the output,
    the source planes.  Returns the frames as the buffers hold them"""
    lay = lay if lay is not None else dk.layout_of(row)
    tag = (row.id,) + tag
    assert dk.kernel_of(row.cs, row.profile, row.w, lay.aligned4, lay.fs, row.tunes, row.out16) == named(row, vw), tag
    assert c.quantizer_info()["mode"] == 3, tag + ("the table is not in LDS",)
    ex = dk.expected(o, row)
    src = laid_out(L, ex.s, row.w, row.h, row.profile, src_lay)
    out = DeviceOut(lay)
    assert all(p % (4 * lay.dtype.itemsize) == (lay.base % 4) * lay.dtype.itemsize for p in out.ptrs()), tag
    before = c.rb_table_info(row.sc)
    assert before["used"] == (row.variant == "rb"), tag + (before,)
    launch(c, src, row.sc, out)
    after = c.rb_table_info(row.sc)
    assert after["table_launches"] - before["table_launches"] == (1 if row.variant == "rb" else 0), tag + (before, after)
    assert after["backoff_launches"] == before["backoff_launches"] == 0, tag + (before, after)
    problem = dk.frames_problem(out.written(), ex.want)
    assert problem is None, tag + (problem,)
    assert src.unchanged(), tag + ("a source plane or a gap changed",)
    return out.frames()


# ---- 1. the matrix
@pytest.mark.parametrize("row", [pytest.param(r, id=r.id) for r in ROWS])
def test_decode_matrix(L, oracle_mod, row):
    held(L, oracle_mod, context(L, row.cfg, row.tunes), row, 4 if row.w % 4 == 0 else 2)


# ---- 2. every kernel in other launch shapes
SHAPES = {"1024_threads": (("block", 1024),), "two_workgroups_of_64": (("grid_dec", 2), ("block", 64))}
GROUPS = [pytest.param(cs, variant, sub, out16, id="%s-%s-%s-%s" % (fk.SPACES[cs][0], variant, "420" if sub else "444", "f16" if out16 else "f32"))
          for (cs, variant) in dk.CASES for sub in (True, False) for out16 in (False, True)]


@pytest.mark.parametrize("cs,variant,sub,out16", GROUPS)
def test_every_kernel_in_other_launch_shapes(L, oracle_mod, cs, variant, sub, out16):
    """k_decode<CS, SUB, 4 and 2, ., ., YT, RB, OUT16> with 1024 threads asked for (block_threads_for may clamp; the kernels are compiled
    for 1024) and as two workgroups of one wave: one unit row per tile, so 2 x 35 tiles per frame of 264x70 and 3 x 3 of 258x6, over three
    or four frames, for two workgroups, the frame changing inside the loop and the last prefetch of each running off the end.  The rows of the matrix with
    preScaling 20, in their own form; the oracle's bytes"""
    rows = [r for r in ROWS if (r.cs, r.variant, r.out16, r.profile, r.sc) == (cs, variant, out16, 2 if sub else 3, 20.0) and (r.w, r.h) in ((264, 70), (258, 6))]
    assert sorted(r.w for r in rows) == [258, 264]
    for row in rows:
        for shape, tunes in SHAPES.items():
            held(L, oracle_mod, context(L, row.cfg, row.tunes + tunes), row, 4 if row.w == 264 else 2, tag=(shape,))


# ---- 3. layouts the vector loads and stores cannot take
LAYOUT_CASES = [(fk.YCC, v, False) for v in ("plain", "yt", "rb")] + [(cs, v, True) for (cs, v) in dk.CASES]
LAYOUT_IDS = ["%s-%s-%s" % (fk.SPACES[cs][0], v, "f16" if out16 else "f32") for (cs, v, out16) in LAYOUT_CASES]


def layout_row(cs, variant, out16, profile, w, h):
    """a row outside the matrix: the packed call with preScaling 20"""
    return dk.Row("%s-%s-%s-p%d-%dx%d" % (fk.SPACES[cs][0], variant, "f16" if out16 else "f32", profile, w, h), cs, variant, dk.cfg_of(cs, profile),
                  dk.tunes_of(cs, variant), profile, w, h, 20.0, "packed", out16)


@pytest.mark.parametrize("kind", ["odd", "half"])
@pytest.mark.parametrize("profile", [0, 1, 2, 3])
@pytest.mark.parametrize("cs,variant,out16", LAYOUT_CASES, ids=LAYOUT_IDS)
def test_source_planes_off_their_alignment(L, oracle_mod, cs, variant, out16, profile, kind):
    """odd: every plane one byte into its buffer, odd row strides, odd frame strides -- a.aligned = 0 and the byte-wise loads, with
    units of four samples (64x32 luma and 4:4:4 chroma), two (its 4:2:0 chroma, 258x6) and one (258x6 4:2:0 chroma), by 8- and 16-bit
    samples.  half: 64x32, the planes half a four-sample unit off (4 bytes off an 8-byte boundary, 2 off 4 for 8-bit samples), strides
    multiples of 8: the four-pixel kernel with aligned = 0.  The output is aligned either way, so the kernel is the aligned launch's"""
    for (w, h) in (((64, 32), (258, 6)) if kind == "odd" else ((64, 32),)):
        row = layout_row(cs, variant, out16, profile, w, h)
        if kind == "odd":
            src_lay = fk.odd_layout(w, h, profile) + (1,)
        else:
            st, base = ms.half_aligned_layout(w, h, profile)
            src_lay = (st, GAP, base)
        hp = ms.HostPlanes([], w, h, profile, *src_lay)
        if kind == "odd":
            assert hp.base % 2 == 1 and all(s % 2 == 1 for s in hp.st) and all(s % 2 == 1 for s in hp.pfs), row.id
        else:
            unit = 8 if profile > 1 else 4
            assert hp.base % unit == unit // 2 and all(s % 8 == 0 for s in tuple(hp.st) + tuple(hp.pfs)), row.id
        held(L, oracle_mod, context(L, row.cfg, row.tunes), row, 4 if w == 64 else 2, src_lay=src_lay, tag=(kind,))


@pytest.mark.parametrize("profile", [0, 1, 2, 3])
@pytest.mark.parametrize("cs,variant,out16", LAYOUT_CASES, ids=LAYOUT_IDS)
def test_outputs_that_take_two_pixels_only(L, oracle_mod, cs, variant, out16, profile):
    """64x32 with the frames two elements into a four-element unit (float: 8 bytes off a 16-byte boundary; binary16: 4 off 8), or
    3 w h + 2 elements apart: decode_impl sends the launch to the two-pixel kernel -- asserted through kernel_of --, which gives the
    frames of the aligned launch and of the oracle"""
    row = layout_row(cs, variant, out16, profile, 64, 32)
    c = context(L, row.cfg, row.tunes)
    aligned = held(L, oracle_mod, c, row, 4, tag=("aligned",))
    for what, base, pad in (("two elements off", 2, 4), ("stride 3wh+2", 4, 2)):
        lay = dk.OutLayout("packed", 3, 64, 32, out16, pad=pad, base=base)
        assert (lay.aligned4, lay.fs % 4) == ((True, 2) if pad == 2 else (False, 0))
        got = held(L, oracle_mod, c, row, 2, lay=lay, tag=(what,))
        assert np.array_equal(got.view(np.uint16 if out16 else np.uint32), aligned.view(np.uint16 if out16 else np.uint32)), (row.id, what)


# ---- 4. a context keeps its state
@pytest.mark.parametrize("cs,variant", dk.CASES, ids=["%s-%s" % (fk.SPACES[cs][0], v) for (cs, v) in dk.CASES])
def test_a_context_keeps_its_state(L, oracle_mod, cs, variant):
    """the same planes decoded twice and once inside begin_unordered(2) / end_unordered, float and binary16 frames: the oracle's bytes
    every time; quantizer_info does not move, rb_table_info counts one table launch per launch of an rb context and nothing else"""
    import torch
    for out16 in (False, True):
        row = layout_row(cs, variant, out16, 2, 264, 70)
        c = context(L, row.cfg, row.tunes)
        ex = dk.expected(oracle_mod, row)
        src = laid_out(L, ex.s, row.w, row.h, row.profile)
        qi, ri = c.quantizer_info(), c.rb_table_info(row.sc)
        call = c.decode_frames_device_f16 if out16 else c.decode_frames_device
        got = []
        for unordered in (False, False, True):
            out = FloatOut(src.nf, row.w, row.h, dtype=np.float16 if out16 else np.float32)
            if unordered:
                c.begin_unordered(2)
            call(src.ptrs, src.st, src.pfs, src.nf, row.w, row.h, row.profile, row.sc, out.ptr, out.fs)
            if unordered:
                c.end_unordered()
            torch.cuda.synchronize()
            got.append(out.frames().view(np.uint16 if out16 else np.float32))
        for k, g in enumerate(got):
            bad = dk.differ(g, ex.want)
            assert not bad.any(), (row.id, "launch %d" % k, np.argwhere(bad)[:4].tolist())
        assert c.quantizer_info() == qi, row.id
        after = c.rb_table_info(row.sc)
        assert after == dict(ri, table_launches=ri["table_launches"] + (3 if variant == "rb" else 0)), (row.id, ri, after)
        assert src.unchanged(), row.id
