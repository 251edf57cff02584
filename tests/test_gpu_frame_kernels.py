"""The plain encode and decode kernels, every instantiation the pickers can return for frames, and the layouts the vector accesses
cannot take -- needs an MI355X.

Every comparison is bit for bit with the oracle (tests/support/frame_kernels.py expected: Oracle.encode of every frame of the launch;
Oracle.decode; lo_pack_plane / lo_unpack_plane); the statistics' sum alone has a bound, rel 1e-4.  Every encode launch has three distinct
frames (log-uniform 1e-4 .. 3e4, special_frame in the corner of 64x32: NaN, infinities, negatives and zeros pass through every
search), row strides 16 bytes wider than the rows, 48 bytes between the frames' planes and 4 floats between the float frames;
planes_problem holds every sample to the oracle's and every other byte of the buffers to the sentinel, and the source frames are
compared with what they were.  The expected planes of 64x32 and 258x6 hold at least 64 distinct sample values each and U differs
from V (asserted on the reference; tests/test_frame_kernels_host.py shows that the comparison rejects planted errors).

k_encode<CS, SUB, VW, LM> (lumahip_pick.hpp pick_enc; the mode is asserted with quantizer_info before anything is compared):
  LM 3 records in LDS          test_encode_matrix[*-m3-*]   PQ-11; YCbCr with statistics (`-stats`)
  LM 5 composite records       test_encode_matrix[ycbcr-m3-*-lm5]   the same YCbCr rows without statistics under "half_table" 0
  LM 4 records in global       test_encode_matrix[*-m4-*]   PQ-11 under "lds_table_max_kb" 0
  LM 7 value-keyed records     test_encode_matrix[*-m7-*]   LINEAR-12
  LM 0 literal, table in LDS   test_encode_matrix[*-m0-*]   PQ-11 under "force_literal" 1; YCbCr: the one frame-fed kernel that stages the
                                                            powf tables and the luminance table (STAGE_LUT | STAGE_POWF)
  LM 2 literal, table global   test_encode_matrix[*-m2-*]   PQ-13 under "force_literal" 1
for CS in Lu'v', RGB, YCbCr (maxLum 1000, colour depth 10, preScaling 1 and 20) and XYZ, SUB by profiles 2 (4:2:0) and 3 (4:4:4), VW 4
at 64x32 where the mode has such a kernel, VW 2 at 258x6 (a ragged last tile) and 6x4: 16 kernels per colour space and the four of
LM 5, 68 in all (tests/test_frame_kernels_host.py derives the set).  RGB and XYZ chroma thereby go through quantize_lut<LM, 1>,
<LM, 2>, <LM, 4> and <LM, 8> for every LM.  The sample size is a kernel argument: profiles 0 and 1 run on one records-in-LDS row per
colour space with an 8-bit table ([*-pq8-*]).  Every row runs the packed float call and one of _planar, _f16, _planar_f16 (the
k_encode<., IN16 = true> twins of pick_enc<true>; the reference is then the oracle on the widened halves), going round so that each
form meets every (colour space, mode); statistics are requested on every other row.  No launch of the matrix takes the half-input
table (half_table_info "table_launches" is read around every row).
  LM 6 half-input table        stays with tests/test_gpu_half_table.py; test_ycbcr_halves_take_the_half_table_when_it_exists records, for
                               the matrix's YCbCr configuration on a default context, that halves without statistics launch it and
                               halves with statistics do not
  the persistent loop          test_encode_two_workgroups_of_one_wave   ("grid_enc" 2, "block" 64) YCbCr LM 0, RGB LM 4, Lu'v' LM 7

Layouts (one records-in-LDS configuration per colour space, profiles 0-3, k_encode and then k_decode on the planes it wrote):
  every base, row stride and frame stride odd     test_fully_unaligned_planes      the six byte-wise branches of store_samples and
                                                                                   load_samples: N = 4, 2, 1 by 8- and 16-bit samples
  good for units of two samples, not of four      test_half_aligned_planes         VW 4 with aligned = 0
  frames 8 bytes off a 16-byte boundary / a frame stride of 3 w h + 2              test_frames_that_take_two_pixels_only (both ways)
  refused before any launch                       test_refused_layouts_write_nothing

k_decode<CS, SUB, 2, GL = true> (and its OUT16 twin), the table in global memory:
  test_decode_with_the_table_in_global_memory     the 13-bit siblings under "lds_table_max_kb" 0, random codes, YCbCr preScaling 20 and
                                                  65537; test_global_decode_two_workgroups_of_one_wave ("grid_dec" 2, "block" 64)

Pack-only and unpack-only (lumahip_pack_frame_host / lumahip_unpack_frame_host: CS_PACK for Lu'v' and YCbCr quantizers, CS_RGB for RGB
and XYZ), modes 3, 0 and 7:   test_pack_only_and_unpack_only

Left unrun: nothing of the above.  The k_decode<CS_PACK, ., ., DISP> and k_encode<CS_PACK, ., ., IN16> instantiations do not exist."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.golden.make_golden import special_frame  # noqa: E402
from tests.support import frame_kernels as fk  # noqa: E402
from tests.support.device import FloatOut, Frames, L, Planes, ctx, from_frames, random_planes  # noqa: E402,F401  (L is the module fixture)
from tests.support.host import ERR_ARG, GAP, float_to_half_np, plane_rows, plane_samples, same_bits, widen_halves  # noqa: E402

NF = fk.NF
GARBAGE = [0xFF, 0xFF, 0x00, 0x00, 0x34, 0x12, 0xFF, 0x7F]     # out-of-range codes, as make_golden.py's decode fixtures hold them
_ctx = {}


def context(L, cfg, tunes=()):
    """a context on torch's stream per (configuration, tunes), made once: the 13-bit record indices are built once per process"""
    key = (cfg, tuple(tunes))
    if key not in _ctx:
        c = ctx(L, cfg)
        for name, v in tunes:
            c.tune(name, v)
        _ctx[key] = c
    return _ctx[key]


def encode_call(c, fr, form, sc, pl, stats):
    """lumahip_encode_frames_device in one of its four forms; the per-frame {sum, min, max} when asked for"""
    import torch
    esz = fr.host.dtype.itemsize
    src = [fr.ptr + k * fr.n * esz for k in range(3)] if form.startswith("planar") else fr.ptr
    suffix = {"packed": "", "planar": "_planar", "f16": "_f16", "planar_f16": "_planar_f16"}[form]
    sd = torch.full((3 * fr.nf,), float("nan"), dtype=torch.float32, device=fr.t.device) if stats else None
    getattr(c, "encode_frames_device" + suffix)(src, fr.fs, fr.nf, fr.w, fr.h, sc, pl.profile, pl.ptrs, pl.st, pl.pfs,
                                                sd.data_ptr() if stats else None)
    torch.cuda.synchronize()
    return sd.cpu().numpy().reshape(fr.nf, 3) if stats else None


def encoded(L, o, c, cfg, profile, w, h, sc, form="packed", stats=False, strides=None, gap=GAP, base=0, fbase=0, fpad=4, tag=()):
    """one encode launch held to the oracle: the planes, every byte around them, the source frames, the statistics; the oracle's planes
    themselves are first held to the conditions on the inputs (fk.informative).
    Returns (the Planes, their host buffers, the oracle's planes and strides)"""
    halves = "f16" in form
    frs, exp, est = fk.expected(o, cfg, profile, w, h, sc, halves)
    if (w, h) != (6, 4):      # (24 samples per plane)
        fk.informative(exp, w, h, profile, tag + (form,))
    fr = Frames(frs, dtype=np.float16 if halves else np.float32, pad=fpad, base=fbase)
    pl = Planes(L, w, h, profile, NF, strides=strides if strides is not None else fk.wide_layout(w, h, profile), gap=gap, base=base)
    got = encode_call(c, fr, form, sc, pl, stats)
    bufs = pl.host()
    problem = fk.planes_problem(bufs, exp, w, h, profile, pl.st, gap, base)
    assert problem is None, tag + (form, problem)
    assert fr.unchanged(), tag + (form, "the source frames changed")
    if stats:
        for f in range(NF):
            want = fk.expected_stats(o, cfg, widen_halves(frs[f]) if halves else frs[f], sc)
            problem = fk.stats_problem(got[f], want)
            assert problem is None, tag + (form, f, problem)
    return pl, bufs, exp, est


def decoded(c, pl, sc, out, f16=False):
    import torch
    call = c.decode_frames_device_f16 if f16 else c.decode_frames_device
    call(pl.ptrs, pl.st, pl.pfs, pl.nf, pl.w, pl.h, pl.profile, sc, out.ptr, out.fs)
    torch.cuda.synchronize()
    return out.frames()


# ---- 1. the encode matrix
@pytest.mark.parametrize("row", [pytest.param(r, id=r[0]) for r in fk.encode_matrix()])
def test_encode_matrix(L, oracle_mod, row):
    ident, cs, mode, cfg, tunes, profile, w, h, sc, stats, form, lm5 = row
    c = context(L, cfg, tunes)
    assert c.quantizer_info()["mode"] == mode
    before = c.half_table_info(sc)["table_launches"]
    _, packed, _, _ = encoded(L, oracle_mod, c, cfg, profile, w, h, sc, "packed", stats, tag=(ident,))
    _, other, _, _ = encoded(L, oracle_mod, c, cfg, profile, w, h, sc, form, stats, tag=(ident,))
    if "f16" not in form:      # (the same frames: the same bytes)
        assert all(np.array_equal(a, b) for a, b in zip(packed, other)), (ident, form)
    assert c.half_table_info(sc)["table_launches"] == before, (ident, "a launch took the half-input table kernel")


@pytest.mark.parametrize("profile,w,h", [(2, 64, 32), (3, 258, 6)])
def test_ycbcr_halves_take_the_half_table_when_it_exists(L, oracle_mod, profile, w, h):
    """a default context: frames of halves without statistics launch k_encode<CS_YCBCR, ., ., 6, true> exactly when half_table_info says
    the table exists and fits; with statistics the row's own mode runs (LM 3).  The same planes either way"""
    cfg, sc = fk.config(fk.YCC, fk.PQ, 11), 20.0
    c = context(L, cfg)
    assert c.quantizer_info()["mode"] == 3
    info = c.half_table_info(sc)
    for form in ("f16", "planar_f16"):
        encoded(L, oracle_mod, c, cfg, profile, w, h, sc, form, False, tag=("halves",))
        after = c.half_table_info(sc)["table_launches"]
        print("%s p%d %dx%d: the half-input table %s, %d launch(es) with it" % (form, profile, w, h, "exists" if info["used"] else "does not exist",
                                                                             after - info["table_launches"]))
        assert after - info["table_launches"] == (1 if info["used"] else 0), form
        encoded(L, oracle_mod, c, cfg, profile, w, h, sc, form, True, tag=("halves", "stats"))
        assert c.half_table_info(sc)["table_launches"] == after, form
        info = c.half_table_info(sc)


LOOPED = [pytest.param(fk.YCC, 0, 20.0, id="ycbcr-m0"), pytest.param(fk.RGB, 4, 1.0, id="rgb-m4"), pytest.param(fk.LUV, 7, 1.0, id="luv-m7")]


@pytest.mark.parametrize("profile,w,h", [(2, 64, 32), (3, 64, 32), (2, 258, 6), (3, 258, 6)])
@pytest.mark.parametrize("cs,mode,sc", LOOPED)
def test_encode_two_workgroups_of_one_wave(L, oracle_mod, cs, mode, sc, profile, w, h):
    """"grid_enc" 2 and "block" 64: one row pair per tile, so two workgroups walk 48 (64x32) or 27 (258x6) tiles across the frame
    boundaries, and the last prefetch of each runs off the end; the bytes of the default launch"""
    ptf, bits, tunes = fk.MODES[mode]
    cfg = fk.config(cs, ptf, bits)
    tag = (cs, mode, profile, w, h)
    _, default, _, _ = encoded(L, oracle_mod, context(L, cfg, tunes), cfg, profile, w, h, sc, "packed", True, tag=tag + ("default",))
    c = context(L, cfg, tunes + (("grid_enc", 2), ("block", 64)))
    assert c.quantizer_info()["mode"] == mode
    for form in ("packed", "f16"):
        _, looped, _, _ = encoded(L, oracle_mod, c, cfg, profile, w, h, sc, form, True, tag=tag)
        if form == "packed":
            assert all(np.array_equal(a, b) for a, b in zip(default, looped)), tag


# ---- 2. layouts the vector accesses cannot take
def layout_cfg(cs, profile):
    return (fk.config(cs, fk.PQ, 11) if profile > 1 else fk.pq8(cs)), fk.SPACES[cs][4][-1]


def decode_held(o, c, cfg, pl, bufs, exp, est, sc, out, tag):
    """the decode of the planes an encode wrote, from where it wrote them: the oracle's floats bit for bit, the planes as they were"""
    got = decoded(c, pl, sc, out)
    for f in range(NF):
        assert same_bits(got[f], fk.oracle(o, cfg).decode(exp[f], est, pl.w, pl.h, sc, pl.profile)), tag + (f, "decoded floats")
    assert all(np.array_equal(a, b) for a, b in zip(pl.host(), bufs)), tag + ("the decode changed a plane",)


@pytest.mark.parametrize("w,h", fk.SIZES)
@pytest.mark.parametrize("profile", [0, 1, 2, 3])
@pytest.mark.parametrize("cs", [fk.LUV, fk.RGB, fk.YCC, fk.XYZ], ids=lambda cs: fk.SPACES[cs][0])
def test_fully_unaligned_planes(L, oracle_mod, cs, profile, w, h):
    """every plane one byte into its buffer, odd row strides, odd frame strides: a.aligned = 0 in k_encode and k_decode, units of four
    samples (64x32 luma and 4:4:4 chroma), two (4:2:0 chroma at 64x32, everything else's luma) and one (4:2:0 chroma of the two-pixel
    kernels), by 8-bit (profiles 0, 1) and 16-bit samples"""
    cfg, sc = layout_cfg(cs, profile)
    c = context(L, cfg)
    st, gap = fk.odd_layout(w, h, profile)
    tag = (fk.SPACES[cs][0], profile, w, h)
    pl, bufs, exp, est = encoded(L, oracle_mod, c, cfg, profile, w, h, sc, strides=st, gap=gap, base=1, tag=tag)
    assert all(p % 2 == 1 for p in pl.ptrs) and all(s % 2 == 1 for s in pl.st) and all(s % 2 == 1 for s in pl.pfs)
    decode_held(oracle_mod, c, cfg, pl, bufs, exp, est, sc, FloatOut(NF, w, h), tag)


@pytest.mark.parametrize("profile", [0, 1, 2, 3])
@pytest.mark.parametrize("cs", [fk.LUV, fk.RGB, fk.YCC, fk.XYZ], ids=lambda cs: fk.SPACES[cs][0])
def test_half_aligned_planes(L, oracle_mod, cs, profile):
    """64x32, planes half a four-sample unit off its alignment (4 bytes off an 8-byte boundary for 16-bit samples, 2 off 4 for 8-bit),
    strides and frame strides multiples of 8: the four-pixel kernels run with aligned = 0"""
    cfg, sc = layout_cfg(cs, profile)
    c = context(L, cfg)
    w, h, base = 64, 32, 4 if profile > 1 else 2
    tag = (fk.SPACES[cs][0], profile, "half-aligned")
    pl, bufs, exp, est = encoded(L, oracle_mod, c, cfg, profile, w, h, sc, base=base, tag=tag)
    assert pl.ptrs[0] % (2 * base) == base and all(s % 8 == 0 for s in pl.st) and all(s % 8 == 0 for s in pl.pfs)
    decode_held(oracle_mod, c, cfg, pl, bufs, exp, est, sc, FloatOut(NF, w, h), tag)


@pytest.mark.parametrize("fbase,fpad", [pytest.param(2, 4, id="8-bytes-off-16"), pytest.param(0, 2, id="stride-3wh+2")])
@pytest.mark.parametrize("profile", [2, 3])
@pytest.mark.parametrize("cs", [fk.LUV, fk.RGB, fk.YCC, fk.XYZ], ids=lambda cs: fk.SPACES[cs][0])
def test_frames_that_take_two_pixels_only(L, oracle_mod, cs, profile, fbase, fpad):
    """64x32 with source and output frames 8 bytes off a 16-byte boundary, or 3 w h + 2 floats apart: check_frame_alignment and
    decode_impl send the launch to the two-pixel kernels; the bytes of the aligned launch, both ways"""
    cfg, sc = layout_cfg(cs, profile)
    c = context(L, cfg)
    w, h = 64, 32
    tag = (fk.SPACES[cs][0], profile, fbase, fpad)
    _, aligned, _, _ = encoded(L, oracle_mod, c, cfg, profile, w, h, sc, tag=tag + ("aligned",))
    pl, bufs, exp, est = encoded(L, oracle_mod, c, cfg, profile, w, h, sc, fbase=fbase, fpad=fpad, tag=tag)
    assert all(np.array_equal(a, b) for a, b in zip(aligned, bufs)), tag
    out = FloatOut(NF, w, h, pad=fpad, base=fbase)
    assert out.ptr % 16 == 4 * fbase and out.fs % 4 == fpad % 4
    decode_held(oracle_mod, c, cfg, pl, bufs, exp, est, sc, out, tag)
    ref = FloatOut(NF, w, h)
    assert same_bits(decoded(c, pl, sc, ref), out.frames()), tag + ("the aligned decode",)


def test_refused_layouts_write_nothing(L, oracle_mod):
    """frames or outputs 4 bytes off an 8-byte boundary, an odd frame stride, a plane row stride below the row: LUMAHIP_ERR_ARG from
    check_layout / check_frame_alignment (encode) and check_layout / decode_impl's alignment test, all in front of the launch; the
    planes and the float output keep their fill"""
    import torch
    cfg, sc, profile, w, h = fk.config(fk.LUV, fk.PQ, 11), 1.0, 2, 64, 32
    c = context(L, cfg)
    frs, exp, est = fk.expected(oracle_mod, cfg, profile, w, h, sc)
    good_st = fk.wide_layout(w, h, profile)
    short = (plane_rows(w, h, profile, 0)[1] - 2,) + good_st[1:]
    short_c = good_st[:2] + (plane_rows(w, h, profile, 2)[1] - 2,)
    src = from_frames(L, exp, w, h, profile, strides=good_st, padding="sentinel")
    for what, fbase, fpad, st in (("4 bytes off an 8-byte boundary", 1, 4, good_st), ("an odd frame stride", 0, 3, good_st),
                                  ("a luma row stride below the row", 0, 4, short), ("a chroma row stride below the row", 0, 4, short_c)):
        fr = Frames(frs, pad=fpad, base=fbase)
        pl = Planes(L, w, h, profile, NF, strides=good_st)
        with pytest.raises(L.LumaHipError) as e:
            c.encode_frames_device(fr.ptr, fr.fs, NF, w, h, sc, profile, pl.ptrs, st, pl.pfs)
        assert e.value.code == ERR_ARG, what
        out = FloatOut(NF, w, h, pad=fpad, base=fbase)
        with pytest.raises(L.LumaHipError) as e:
            c.decode_frames_device(src.ptrs, st, src.pfs, NF, w, h, profile, sc, out.ptr, out.fs)
        assert e.value.code == ERR_ARG, what
        torch.cuda.synchronize()
        assert pl.unchanged() and out.untouched() and fr.unchanged() and src.unchanged(), what
    encoded(L, oracle_mod, c, cfg, profile, w, h, sc, tag=("after the refused calls",))


# ---- 3. plain decode with the table in global memory
GLOBAL_ROWS = [pytest.param(fk.LUV, 1.0, id="luv"), pytest.param(fk.RGB, 1.0, id="rgb"), pytest.param(fk.XYZ, 1.0, id="xyz"),
               pytest.param(fk.YCC, 20.0, id="ycbcr-sc20"), pytest.param(fk.YCC, 65537.0, id="ycbcr-sc65537")]
GLOBAL_TUNES = (("lds_table_max_kb", 0),)


def global_decode(L, o, c, cfg, profile, w, h, sc, tag):
    """three frames of random codes through the float and the binary16 decode; returns the float frames"""
    assert c.quantizer_info()["mode"] == 4          # the 13-bit table's records are in global memory, as the table is
    pl = random_planes(L, np.random.default_rng(1000 * w + 10 * h + profile), w, h, profile, NF)
    host = pl.host()
    want = np.stack([fk.oracle(o, cfg).decode(pl.frame(host, f), pl.st, w, h, sc, profile) for f in range(NF)])
    got = decoded(c, pl, sc, FloatOut(NF, w, h))
    assert same_bits(got, want), tag + ("floats",)
    got16 = decoded(c, pl, sc, FloatOut(NF, w, h, dtype=np.float16), f16=True)
    assert np.array_equal(got16.view(np.uint16), float_to_half_np(want)), tag + ("halves",)
    assert pl.unchanged(), tag + ("a code plane changed",)
    return got


@pytest.mark.parametrize("w,h", [(64, 32), (258, 6)])
@pytest.mark.parametrize("profile", [2, 3])
@pytest.mark.parametrize("cs,sc", GLOBAL_ROWS)
def test_decode_with_the_table_in_global_memory(L, oracle_mod, cs, sc, profile, w, h):
    cfg = fk.pq13(cs)
    global_decode(L, oracle_mod, context(L, cfg, GLOBAL_TUNES), cfg, profile, w, h, sc, (fk.SPACES[cs][0], sc, profile, w, h))


@pytest.mark.parametrize("w,h", [(64, 32), (258, 6)])
def test_global_decode_two_workgroups_of_one_wave(L, oracle_mod, w, h):
    """"grid_dec" 2 and "block" 64 on the YCbCr row: the persistent loop runs and changes frame inside it; the default launch's floats"""
    cfg, sc, profile = fk.pq13(fk.YCC), 20.0, 2
    default = global_decode(L, oracle_mod, context(L, cfg, GLOBAL_TUNES), cfg, profile, w, h, sc, ("default", w, h))
    looped = global_decode(L, oracle_mod, context(L, cfg, GLOBAL_TUNES + (("grid_dec", 2), ("block", 64))), cfg, profile, w, h, sc, ("looped", w, h))
    assert same_bits(looped, default)


# ---- 4. pack-only and unpack-only
PACK_TABLES = [pytest.param(fk.PQ, 11, (), 3, (2, 3), id="pq11-m3"), pytest.param(fk.PQ, 8, (), 3, (0, 1, 2, 3), id="pq8-m3"),
               pytest.param(fk.PQ, 11, (("force_literal", 1),), 0, (2, 3), id="pq11-m0"),
               pytest.param(fk.PQ, 8, (("force_literal", 1),), 0, (0, 1, 2, 3), id="pq8-m0"), pytest.param(fk.LINEAR, 12, (), 7, (2, 3), id="linear12-m7")]


def transformed_frame(o, cfg, w, h, sc):
    """an oracle-transformed frame, special_frame in its corner, and in its last row values above the table's top and below zero
    in all three channels"""
    orc = fk.oracle(o, cfg)
    t = np.array(fk.frames(w, h, 1)[0], copy=True)
    orc.transform(t, True, sc)
    sp = special_frame(8, 16) if h >= 8 else special_frame(4, 16)
    t[:, :sp.shape[1], :16] = sp
    top = float(orc.mapping[-1])
    t[:, h - 1, w - 6:] = np.array([2 * top, np.nextafter(np.float32(top), np.float32(np.inf)), -1.0, -top, 1e38, -1e-3], dtype=np.float32)
    return t


@pytest.mark.parametrize("ptf,bits,tunes,mode,profiles", PACK_TABLES)
@pytest.mark.parametrize("cs", [fk.LUV, fk.RGB, fk.YCC, fk.XYZ], ids=lambda cs: fk.SPACES[cs][0])
def test_pack_only_and_unpack_only(L, oracle_mod, cs, ptf, bits, tunes, mode, profiles):
    """the reference is lo_pack_plane / lo_unpack_plane plane by plane; the unpacked planes also hold out-of-range codes"""
    cfg = fk.config(cs, ptf, bits)
    c = context(L, cfg, tunes)
    assert c.quantizer_info()["mode"] == mode
    orc = fk.oracle(oracle_mod, cfg)
    for profile in profiles:
        for (w, h) in ((64, 32), (258, 6)):
            tag = (fk.SPACES[cs][0], mode, profile, w, h)
            t = transformed_frame(oracle_mod, cfg, w, h, fk.SPACES[cs][4][-1])
            planes, st, _ = c.pack_frame(t.copy(), profile)
            want = [np.zeros_like(p) for p in planes]
            for p in range(3):
                orc.L.lo_pack_plane(C.byref(orc.q), t[p].ctypes.data, p, profile, w, h, want[p].ctypes.data, st[p], None)
                assert np.array_equal(planes[p], want[p]), tag + (p, "packed")
            assert np.unique(plane_samples(want[0], w, h, profile, 0)).size >= fk.MIN_DISTINCT and not np.array_equal(want[1], want[2]), tag
            for p in want:
                n = min(len(GARBAGE), plane_rows(w, h, profile, 0)[1] // 2)
                p[1, :n] = GARBAGE[:n]
            assert same_bits(c.unpack_frame(want, st, w, h, profile), orc.unpack(want, st, w, h, profile)), tag + ("unpacked",)
