"""Content light level (include/lumahip_compare.h): lumahip_light_level_frames_device in its four forms, lumahip_planes_light_level_frames_device
and the two host forms -- per frame the eight integer words MaxCLL and MaxFALL are made of.  Every expectation is exact equality of
integers with the numpy model (tests/support/light_level.py, which tests/test_light_level_host.py holds to a scalar restatement); before
every call the output holds the 0xC3 pattern with 16 guard words behind it, which must survive; the inputs and the sentinel bytes around
them must be as they were after every case.

1. Frame-fed against the model: sizes (6,4) (34,18) (258,6) (260,6) (264,70) (64,32) x 3 distinct frames with a gap between them x scale
   1, 20, 0.01, packed and planar, floats, and halves held to the float call on the widened frames; frame 0 holds the planted pixels
   (one channel NaN, all three NaN, +inf, -inf, negatives, -0, a denormal, 16777216.0 and the float below it); a frame base 8 bytes
   off 16-byte alignment (halves: 4 off 8).
2. Plane-fed: the CFG configurations with tables of at most 12 bits, all four colour spaces, profiles 0-3, sc 1, 20, 0.01, scale 1 and
   sc: the model on the ORACLE's decode of the same planes, and the frame-fed call on what lumahip_decode_frames_device wrote; planes
   with odd bases and strides (byte-wise loads); random planes with out-of-range codes; pq14_luv8 is LUMAHIP_ERR_UNSUPPORTED.
3. Launch shapes: default, two workgroups of one wave, 1024 threads asked for.
4. Context: no quantizer for the frame-fed calls, LUMAHIP_ERR_STATE for the plane-fed one; the quantizer untouched; a 720p frame twice
   and in an unordered section; both host forms.
5. Refusals, each before any launch, leaving the output untouched.
"""
import numpy as np
import pytest

from tests.support.device import FloatOut, Frames, L, Planes, ctx, from_frames, random_planes, table_for  # noqa: F401  (L is the module fixture)
from tests.support.frame_kernels import odd_layout
from tests.support.host import CFG, ERR_ARG, ERR_STATE, ERR_UNSUPPORTED, OUT_FILL, SENTINEL, float_frames, planes_from_frames
from tests.support.light_level import LL_SIZES, NF, SCALES, WORDS, frames, light, light_buf, light_words, model, model_frames, planes_light

pytestmark = pytest.mark.gpu

LDS_CONFIGS = [n for n in CFG if n != "pq14_luv8"]
PLANE_SIZES = [(34, 18), (264, 70), (258, 6), (64, 32)]     # two pixels per thread, four over several tiles, two ragged, four in one tile


def bare(L):
    """a context that never had a quantizer set"""
    return ctx(L, None, quantizer=False)


def oracle(o, name):
    return o.Oracle(*CFG[name], table=table_for(o, CFG[name]))


def oracle_planes(orc, fr, sc, profile):
    """the oracle's planes of the frames, per frame three (rows, stride) arrays, and their strides"""
    out, st = [], None
    for f in fr:
        pl, st, _ = orc.encode(f.copy(), sc, profile)
        out.append(pl)
    return out, tuple(int(s) for s in st)


def decoded_words(orc, pl, sc, scale):
    """the model on the oracle's decode of the device planes `pl`"""
    host = pl.host()
    return model_frames([orc.decode(pl.frame(host, f), pl.st, pl.w, pl.h, sc, pl.profile) for f in range(pl.nf)], scale)


def via_decode(c, cmp_ctx, pl, sc, scale):
    """the frame-fed call of cmp_ctx on what lumahip_decode_frames_device of c wrote for the planes"""
    import torch
    out = FloatOut(pl.nf, pl.w, pl.h)
    c.decode_frames_device(pl.ptrs, pl.st, pl.pfs, pl.nf, pl.w, pl.h, pl.profile, sc, out.ptr, out.fs)
    torch.cuda.synchronize()
    return light(cmp_ctx, out, scale)


# ---- 1. frame-fed against the model
@pytest.mark.parametrize("w,h", LL_SIZES)
def test_frames_equal_the_model(L, w, h):
    c = bare(L)
    fr, fr16 = frames(w, h), frames(w, h, halves=True)
    d32, d32off = Frames(fr), Frames(fr, base=2)
    w32, d16, d16off = Frames(fr16), Frames(fr16, dtype=np.float16), Frames(fr16, dtype=np.float16, base=2)
    assert d32.fs > 3 * w * h and d32off.ptr % 16 == 8 and d16off.ptr % 8 == 4
    for scale in SCALES:
        want, want16 = model_frames(fr, scale), model_frames(fr16, scale)
        tag = (w, h, scale)
        assert want[0, 3] > 0 and want[0, 2] > 0 and not want[1:, 2:4].any(), tag
        for form in ("packed", "planar"):
            assert np.array_equal(light(c, d32, scale, form), want), tag + (form, light(c, d32, scale, form), want)
            assert np.array_equal(light(c, d32off, scale, form), want), tag + (form, "off 16-byte alignment")
            assert np.array_equal(light(c, w32, scale, form), want16), tag + (form, "widened halves")
        for form in ("f16", "planar_f16"):
            assert np.array_equal(light(c, d16, scale, form), want16), tag + (form, light(c, d16, scale, form), want16)
            assert np.array_equal(light(c, d16off, scale, form), want16), tag + (form, "off 8-byte alignment")
    for d in (d32, d32off, w32, d16, d16off):
        assert d.unchanged(), (w, h, "an input frame or a byte around it changed")


# ---- 2. plane-fed
@pytest.mark.parametrize("name", LDS_CONFIGS)
def test_planes_equal_the_model_on_the_oracles_decode_and_the_frame_fed_call_on_the_decode_calls_frames(L, oracle_mod, name):
    c, cmp_ctx, orc = ctx(L, CFG[name]), bare(L), oracle(oracle_mod, name)
    rng = np.random.default_rng(len(name) * 7 + CFG[name][1])
    n = 0
    for profile in range(4):
        for sc in SCALES:
            w, h = PLANE_SIZES[n % len(PLANE_SIZES)]
            n += 1
            src = float_frames(rng, NF, w, h)
            enc, st = oracle_planes(orc, src, sc, profile)
            pl = from_frames(L, enc, w, h, profile, strides=st, padding="sentinel")
            before = pl.host()
            for scale in sorted({1.0, sc}):
                tag = (name, profile, sc, scale, w, h)
                got = planes_light(c, pl, sc, scale)
                want = decoded_words(orc, pl, sc, scale)
                assert np.array_equal(got, want), tag + (got, want)
                assert np.array_equal(got, via_decode(c, cmp_ctx, pl, sc, scale)), tag + ("the decode call's frames",)
                # (8-bit samples keep the low byte of wider codes: such planes decode to anything, and only need to be measured alike)
                if profile > 1 or CFG[name][1] <= 8:
                    assert got[:, 0].all() and got[:, 4].all() and len({int(x) for x in got[:, 0]}) == NF, tag + ("frames without light", got)
            assert all(np.array_equal(a, b) for a, b in zip(before, pl.host())) and pl.gaps_intact(before), (name, profile, sc)
    assert n == 12


def odd_planes(L, enc, w, h, profile):
    """the frames in planes whose bases, row strides and frame strides are odd: every load byte by byte"""
    st, gaps = odd_layout(w, h, profile)
    fill = planes_from_frames(enc, w, h, profile, st, "sentinel", gaps, 1)
    pl = Planes(L, w, h, profile, len(enc), fill=fill, strides=st, gap=gaps, base=1)
    assert all(p % 2 == 1 for p in pl.ptrs) and all(s % 2 == 1 for s in pl.st) and all(s % 2 == 1 for s in pl.pfs)
    return pl


@pytest.mark.parametrize("name", ["pq11_luv8", "pq10_ycbcr10", "pq12_rgb", "linear12_xyz"])
def test_planes_with_odd_bases_and_strides_and_random_planes(L, oracle_mod, name):
    c, cmp_ctx, orc = ctx(L, CFG[name]), bare(L), oracle(oracle_mod, name)
    sc = 20.0 if CFG[name][2] == 2 else 1.0
    rng = np.random.default_rng(len(name))
    for profile in (2, 3, 0):
        for (w, h) in ((264, 70), (34, 18)):
            enc, st = oracle_planes(orc, float_frames(rng, NF, w, h), sc, profile)
            aligned = from_frames(L, enc, w, h, profile, strides=st, padding="sentinel")
            odd = odd_planes(L, enc, w, h, profile)
            before = odd.host()
            want = decoded_words(orc, aligned, sc, sc)
            tag = (name, profile, w, h)
            assert np.array_equal(planes_light(c, aligned, sc, sc), want), tag
            assert np.array_equal(planes_light(c, odd, sc, sc), want), tag + ("odd",)
            assert all(np.array_equal(a, b) for a, b in zip(before, odd.host())) and odd.gaps_intact(before), tag
            # random bytes: codes beyond every table
            rnd = random_planes(L, rng, w, h, profile, NF)
            got = planes_light(c, rnd, sc, sc)
            assert np.array_equal(got, decoded_words(orc, rnd, sc, sc)), tag + ("random planes",)
            assert np.array_equal(got, via_decode(c, cmp_ctx, rnd, sc, sc)), tag + ("random planes, the decode call's frames",)
            assert rnd.unchanged(), tag


def test_tables_beyond_12_bits_are_unsupported(L):
    import torch
    c = ctx(L, CFG["pq14_luv8"])
    w, h, profile = 64, 32, 2
    pl = Planes(L, w, h, profile, 1)
    o = light_buf(1)
    with pytest.raises(L.LumaHipError) as e:
        c.planes_light_level_frames_device(pl.ptrs, pl.st, pl.pfs, 1, w, h, profile, 1.0, 1.0, o.data_ptr())
    assert e.value.code == ERR_UNSUPPORTED, e.value
    torch.cuda.synchronize()
    assert np.all(o.cpu().numpy() == OUT_FILL) and pl.unchanged()
    # ... while the frame-fed calls do not ask about the quantizer
    fr = frames(w, h)
    assert np.array_equal(light(c, Frames(fr), 1.0), model_frames(fr, 1.0))


# ---- 3. launch shapes
def shaped(L, cfg=None):
    out = {}
    for shape in ("default", "two_workgroups_of_64", "1024_threads"):
        c = ctx(L, cfg) if cfg is not None else bare(L)
        if shape == "two_workgroups_of_64":      # the persistent loop across frames: flushes inside it
            c.tune("block", 64)
            c.tune("grid_enc", 2)
        elif shape == "1024_threads":            # (the YCbCr plane-fed kernels: clamped to their 512)
            c.tune("block", 1024)
        out[shape] = c
    return out


def test_launch_shapes_give_identical_words_frames(L):
    shapes = shaped(L)
    for (w, h) in ((264, 70), (258, 6), (34, 18)):
        fr = frames(w, h, halves=True)
        d32, d16 = Frames(fr), Frames(fr, dtype=np.float16)
        want = model_frames(fr, 20.0)
        for shape, c in shapes.items():
            assert np.array_equal(light(c, d32, 20.0), want), (w, h, shape)
            assert np.array_equal(light(c, d16, 20.0, "planar_f16"), want), (w, h, shape, "halves")


@pytest.mark.parametrize("name", ["pq11_luv8", "pq10_ycbcr10", "linear12_xyz"])
def test_launch_shapes_give_identical_words_planes(L, oracle_mod, name):
    shapes, orc = shaped(L, CFG[name]), oracle(oracle_mod, name)
    sc = 20.0 if CFG[name][2] == 2 else 1.0
    rng = np.random.default_rng(3)
    for profile, (w, h) in ((2, (264, 70)), (3, (258, 6)), (0, (34, 18))):
        enc, st = oracle_planes(orc, float_frames(rng, NF, w, h), sc, profile)
        pl = from_frames(L, enc, w, h, profile, strides=st, padding="sentinel")
        want = decoded_words(orc, pl, sc, sc)
        for shape, c in shapes.items():
            assert np.array_equal(planes_light(c, pl, sc, sc), want), (name, profile, w, h, shape)


# ---- 4. context
def test_the_plane_fed_call_needs_the_quantizer_and_leaves_it_alone(L, oracle_mod):
    import torch
    w, h, profile = 64, 32, 2
    pl = Planes(L, w, h, profile, 1)
    o = light_buf(1)
    with pytest.raises(L.LumaHipError) as e:
        bare(L).planes_light_level_frames_device(pl.ptrs, pl.st, pl.pfs, 1, w, h, profile, 1.0, 1.0, o.data_ptr())
    assert e.value.code == ERR_STATE, e.value
    torch.cuda.synchronize()
    assert np.all(o.cpu().numpy() == OUT_FILL)
    # a context with both quantizers: its info and its encode are the same before and after both families
    c = ctx(L, CFG["pq10_ycbcr10"], CFG["pq11_luv8"])
    fr = frames(w, h)
    d = Frames(fr)
    info = c.quantizer_info()
    enc = Planes(L, w, h, profile, NF)
    c.encode_frames_device(d.ptr, d.fs, NF, w, h, 20.0, profile, enc.ptrs, enc.st, enc.pfs)
    torch.cuda.synchronize()
    before = enc.host()
    assert np.array_equal(light(c, d, 20.0), model_frames(fr, 20.0))
    assert np.array_equal(planes_light(c, enc, 20.0, 20.0), decoded_words(oracle(oracle_mod, "pq10_ycbcr10"), enc, 20.0, 20.0))
    again = Planes(L, w, h, profile, NF)
    c.encode_frames_device(d.ptr, d.fs, NF, w, h, 20.0, profile, again.ptrs, again.st, again.pfs)
    torch.cuda.synchronize()
    assert all(np.array_equal(a, b) for a, b in zip(before, again.host())) and c.quantizer_info() == info


def test_one_720p_frame_twice_and_in_an_unordered_section(L, oracle_mod):
    import torch
    w, h, profile, sc = 1280, 720, 2, 1.0
    c, orc = ctx(L, CFG["pq11_luv8"]), oracle(oracle_mod, "pq11_luv8")
    fr = frames(w, h)[:1]
    d = Frames(fr)
    enc, st = oracle_planes(orc, float_frames(np.random.default_rng(720), 1, w, h), sc, profile)
    pl = from_frames(L, enc, w, h, profile, strides=st, padding="sentinel")
    before = pl.host()
    want_f, want_p = model_frames(fr, 20.0), decoded_words(orc, pl, sc, 20.0)
    for _ in range(2):
        assert np.array_equal(light(c, d, 20.0), want_f)
        assert np.array_equal(planes_light(c, pl, sc, 20.0), want_p)
    outs = [(light_buf(1), light_buf(1)) for _ in range(2)]
    torch.cuda.synchronize()
    c.begin_unordered(2)
    for of, op in outs:
        c.light_level_frames_device(d.ptr, d.fs, 1, w, h, 20.0, of.data_ptr())
        c.planes_light_level_frames_device(pl.ptrs, pl.st, pl.pfs, 1, w, h, profile, sc, 20.0, op.data_ptr())
    c.end_unordered()
    c.sync()
    torch.cuda.synchronize()
    for of, op in outs:
        assert np.array_equal(light_words(of, 1), want_f) and np.array_equal(light_words(op, 1), want_p)
    assert d.unchanged() and all(np.array_equal(a, b) for a, b in zip(before, pl.host())) and pl.gaps_intact(before)


@pytest.mark.parametrize("name", ["pq11_luv8", "pq10_ycbcr10"])
def test_host_forms(L, oracle_mod, name):
    c, orc = ctx(L, CFG[name]), oracle(oracle_mod, name)
    sc = 20.0 if CFG[name][2] == 2 else 1.0
    rng = np.random.default_rng(5)
    for (w, h), profile in (((264, 70), 2), ((34, 18), 1)):
        fr = frames(w, h)
        for f in range(NF):
            keep = fr[f].copy()
            got = c.light_level_frame(fr[f], sc)
            assert got.dtype == np.uint64 and got.shape == (WORDS,) and np.array_equal(got, model(fr[f], sc)), (name, w, h, f)
            assert np.array_equal(fr[f], keep, equal_nan=True)
        assert np.array_equal(bare(L).light_level_frame(fr[1], 0.01), model(fr[1], 0.01))
        enc, st = oracle_planes(orc, float_frames(rng, 1, w, h), sc, profile)
        keep = [p.copy() for p in enc[0]]
        got = c.planes_light_level_frame(enc[0], st, w, h, sc, profile, sc)
        want = model(orc.decode(enc[0], st, w, h, sc, profile), sc)
        assert got.dtype == np.uint64 and got.shape == (WORDS,) and np.array_equal(got, want), (name, w, h, profile, got, want)
        assert all(np.array_equal(a, b) for a, b in zip(enc[0], keep))
        assert L.content_light_level(got, w, h) == L.content_light_level([want], w, h)
    # a refused host call leaves the caller's words alone
    out = np.full(WORDS, OUT_FILL, dtype=np.int64)
    rgb = np.zeros((3, 4, 6), dtype=np.float32)
    assert c.L.lumahip_light_level_frame_host(c.h, rgb.ctypes.data, 6, 4, 0.0, out.ctypes.data) == ERR_ARG and np.all(out == OUT_FILL)
    assert c.L.lumahip_light_level_frame_host(c.h, rgb.ctypes.data, 5, 4, 1.0, out.ctypes.data) == ERR_ARG and np.all(out == OUT_FILL)
    assert c.L.lumahip_light_level_frame_host(c.h, rgb.ctypes.data, 6, 4, 1.0, out.ctypes.data) == 0 and not out.any()


# ---- 5. refusals: nothing is launched, the output is left as it was
def test_refusals_leave_the_output_untouched(L):
    import torch
    w, h, profile, nf = 64, 32, 2, 2
    c = ctx(L, CFG["pq11_luv8"])
    fr = Frames(frames(w, h)[:nf])
    fr16 = Frames(frames(w, h, halves=True)[:nf], dtype=np.float16)
    pl = Planes(L, w, h, profile, nf)
    n = w * h

    def refused(call, args, out_ptr="own"):
        buf = light_buf(nf)
        ptr = buf.data_ptr() if out_ptr == "own" else out_ptr(buf)
        with pytest.raises(L.LumaHipError) as e:
            getattr(c, call)(*args, ptr)
        assert e.value.code == ERR_ARG, (call, args, e.value)
        assert c.L.lumahip_last_error(c.h).decode() != ""
        torch.cuda.synchronize()
        assert np.all(buf.cpu().numpy() == OUT_FILL), (call, args, "an error return wrote to the output or to the guard words behind it")
        assert fr.unchanged() and fr16.unchanged() and pl.unchanged()

    def frame_args(d, planar, esz, w=w, h=h, nf=nf, scale=1.0, ptr=None, fs=None):
        base = d.ptr if ptr is None else ptr
        return ([base + k * n * esz for k in range(3)] if planar else base, d.fs if fs is None else fs, nf, w, h, scale)

    def plane_args(w=w, h=h, nf=nf, profile=profile, scale=1.0, ptrs=None, st=None):
        return (pl.ptrs if ptrs is None else ptrs, pl.st if st is None else st, pl.pfs, nf, w, h, profile, 1.0, scale)

    forms = [("light_level_frames_device", fr, False, 4), ("light_level_frames_device_planar", fr, True, 4),
             ("light_level_frames_device_f16", fr16, False, 2), ("light_level_frames_device_planar_f16", fr16, True, 2)]
    bad_scales = (0.0, -1.0, float("inf"), float("nan"))
    for call, d, planar, esz in forms:
        refused(call, frame_args(d, planar, esz), out_ptr=lambda o: None)                      # a null output
        refused(call, frame_args(d, planar, esz), out_ptr=lambda o: o.data_ptr() + 4)          # a misaligned output
        refused(call, frame_args(d, planar, esz), out_ptr=lambda o: d.ptr + 64)                # an output inside the frames
        refused(call, frame_args(d, planar, esz), out_ptr=lambda o: d.ptr - 8 * (nf * WORDS - 1))   # ... reaching into them from in front
        refused(call, frame_args(d, planar, esz), out_ptr=lambda o: d.ptr + (d.fs + 3 * n - 2) * esz // 8 * 8)   # ... in the last frame's last plane
        refused(call, frame_args(d, planar, esz, w=63))                                        # odd w
        refused(call, frame_args(d, planar, esz, h=31))                                        # odd h
        refused(call, frame_args(d, planar, esz, w=0))
        refused(call, frame_args(d, planar, esz, nf=0))                                        # no frame
        for s in bad_scales:
            refused(call, frame_args(d, planar, esz, scale=s))
        refused(call, frame_args(d, planar, esz, ptr=d.ptr + esz))                             # frames off the two-pixel alignment
        refused(call, frame_args(d, planar, esz, fs=d.fs + 1))                                 # an odd frame stride
    refused("light_level_frames_device", (None, fr.fs, nf, w, h, 1.0))                         # null frames
    refused("light_level_frames_device_planar", ([fr.ptr, None, fr.ptr + 8 * n], fr.fs, nf, w, h, 1.0))
    refused("planes_light_level_frames_device", plane_args(), out_ptr=lambda o: None)
    refused("planes_light_level_frames_device", plane_args(), out_ptr=lambda o: o.data_ptr() + 4)
    refused("planes_light_level_frames_device", plane_args(), out_ptr=lambda o: pl.ptrs[0] + 64)   # an output inside a plane
    refused("planes_light_level_frames_device", plane_args(), out_ptr=lambda o: pl.ptrs[2] - 40)   # ... reaching into one
    refused("planes_light_level_frames_device", plane_args(w=63))
    refused("planes_light_level_frames_device", plane_args(h=31))
    refused("planes_light_level_frames_device", plane_args(nf=0))
    for s in bad_scales:
        refused("planes_light_level_frames_device", plane_args(scale=s))
    refused("planes_light_level_frames_device", plane_args(ptrs=[pl.ptrs[0], None, pl.ptrs[2]]))   # a null plane
    refused("planes_light_level_frames_device", plane_args(profile=4))                             # a bad profile
    refused("planes_light_level_frames_device", plane_args(profile=-1))
    refused("planes_light_level_frames_device", plane_args(st=(pl.st[0], pl.st[1] // 4, pl.st[2])))   # a stride below the row
    # ... and the same arguments are accepted
    assert np.array_equal(light(c, fr, 1.0), model_frames(frames(w, h)[:nf], 1.0))
    assert planes_light(c, pl, 1.0, 1.0).shape == (nf, WORDS)
    assert np.all(pl.host()[0] == SENTINEL)
