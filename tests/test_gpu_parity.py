"""Parity of the HIP path (through the C ABI of liblumahip.so) with the CPU oracle -- needs an MI355X.

Bar: integer Y/U/V planes bit-exact; decoded floats bit-exact as well (tolerance stated per test: 0 ulp,
north_star allows 1), NaN == NaN.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.golden.make_golden import CONFIGS, extreme_frame, special_frame  # noqa: E402
from tests.support.device import L, pair  # noqa: E402,F401  (L is the module fixture)
from tests.support.display import check_rgba, display_bytes, display_t  # noqa: E402
from tests.support.host import same_bits  # noqa: E402


def ulp_diff(a, b):
    a = np.asarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    b = np.asarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7fffffff), a)
    b = np.where(b < 0, -(b & 0x7fffffff), b)
    return np.abs(a - b)


def frames(o, w, h):
    rng = np.random.default_rng(w * 131 + h)
    f = np.exp(rng.uniform(np.log(1e-4), np.log(3e4), size=(3, h, w))).astype(np.float32)
    sp = special_frame(8, 16)
    if h >= 8 and w >= 16:
        f[:, :8, :16] = sp
    return [f, o.synth_frame(w, h, frame=5)]


SIZES = [(16, 8), (64, 32), (66, 34), (258, 6), (2, 2), (4, 2), (320, 180), (1280, 720)]


@pytest.mark.parametrize("name", list(CONFIGS))
@pytest.mark.parametrize("profile", [0, 1, 2, 3])
def test_encode_planes_bit_exact(L, oracle_mod, name, profile):
    o = oracle_mod
    cfg = CONFIGS[name]
    q, orc = pair(L, o, cfg)
    for (w, h) in SIZES[:6] if profile != 2 else SIZES:
        for f in frames(o, w, h):
            for sc in ((1.0, 20.0) if (w, h) == (64, 32) else (1.0,)):
                planes, st, mean = q.ctx.encode_frame(f, sc, profile)
                g = f.copy()
                eplanes, est, eavg = orc.encode(g, sc, profile, threads=4 if w >= 320 else 1)
                assert tuple(st) == tuple(est)
                for p in range(3):
                    assert np.array_equal(planes[p], eplanes[p]), (name, profile, w, h, sc, p)
                if np.isfinite(eavg):
                    assert mean == pytest.approx(eavg, rel=1e-3)


@pytest.mark.parametrize("name", list(CONFIGS))
@pytest.mark.parametrize("profile", [0, 1, 2, 3])
def test_decode_floats_bit_exact(L, oracle_mod, name, profile):
    o = oracle_mod
    cfg = CONFIGS[name]
    q, orc = pair(L, o, cfg)
    rng = np.random.default_rng(99)
    for (w, h) in SIZES[:7]:
        _, hs, st, bps = L.plane_geometry(w, h, profile)
        ws = (w, w // 2 if profile in (0, 2) else w, w // 2 if profile in (0, 2) else w)
        planes = []
        for p in range(3):
            hi = (1 << cfg[1]) if (p == 0 or cfg[2] in (o.CS_RGB, o.CS_XYZ)) else (1 << cfg[3])
            hi = min(hi + 3, 256 if bps == 1 else 65536)   # a few out-of-range codes as well
            codes = rng.integers(0, hi, size=(hs[p], ws[p]))
            buf = np.zeros((hs[p], st[p]), dtype=np.uint8)
            if bps == 2:
                buf[:, :2 * ws[p]] = codes.astype("<u2").view(np.uint8).reshape(hs[p], 2 * ws[p])
            else:
                buf[:, :ws[p]] = codes.astype(np.uint8)
            planes.append(buf)
        for sc in (1.0, 20.0):
            got = q.ctx.decode_frame(planes, st, w, h, sc, profile)
            exp = orc.decode(planes, st, w, h, sc, profile)
            assert same_bits(got, exp), (name, profile, w, h, sc, int(ulp_diff(got, exp).max()))  # tolerance: 0 ulp


@pytest.mark.parametrize("name", list(CONFIGS))
@pytest.mark.parametrize("sc", [1.0, 20.0, 0.25])
def test_transform_color_space_golden(L, oracle_mod, golden_dir, name, sc):
    """LumaQuantizer::transformColorSpace on the GPU against the fixtures generated from the real reference"""
    t = np.load(os.path.join(golden_dir, "ref_transform.npz"))
    q, _ = pair(L, oracle_mod, CONFIGS[name])
    f = t["input"].copy()
    assert q.transformColorSpace(f, True, sc)
    assert same_bits(f, t["%s_fwd_sc%g" % (name, sc)])
    g = t["%s_inv_in_sc%g" % (name, sc)].copy()
    assert q.transformColorSpace(g, False, sc)
    assert same_bits(g, t["%s_inv_sc%g" % (name, sc)])


@pytest.mark.parametrize("name", list(CONFIGS))
def test_quantize_dequantize_arrays_golden(L, oracle_mod, golden_dir, name):
    g = np.load(os.path.join(golden_dir, "ref_quantize.npz"))
    cfg = CONFIGS[name]
    q, _ = pair(L, oracle_mod, cfg)
    assert np.array_equal(q.quantize(g[name + "_in0"], 0).astype(np.uint16), g[name + "_q0"])
    assert np.array_equal(q.quantize(g[name + "_in1"], 1).astype(np.uint16), g[name + "_q1"])
    codes = np.arange(-2, 2 ** cfg[1] + 2, dtype=np.float32)
    assert same_bits(q.dequantize(codes, 0), g[name + "_dq0"])
    assert same_bits(q.dequantize(np.arange(0, 2 ** cfg[3], dtype=np.float32), 1), g[name + "_dq1"])


def test_literal_and_global_lut_modes(L, oracle_mod):
    """a non-monotone table must take the literal bisection path; a 13-bit table has 136 KiB of records (LDS, one
    workgroup per CU) or, with a lower LDS limit, reads them from global memory; all bit-exact against the oracle's
    (literal) search"""
    o = oracle_mod
    rng = np.random.default_rng(5)
    # (a) non-monotone 11-bit table, as a decoder may be handed in attachment 434
    q = L.LumaQuantizer()
    lut = L.build_lut(L.PTF_PQ, 11).copy()
    lut[700:720] = lut[700:720][::-1]
    lut[5] = lut[4]
    q.setQuantizer(L.PTF_PQ, 11, L.CS_LUV, 8, 1e4, 0.005, mapping_override=lut)
    assert q.ctx.quantizer_info()["mode"] == 0
    orc = o.Oracle(o.PTF_PQ, 11, o.CS_LUV, 8, 1e4, 0.005)
    orc.overwrite_mapping(lut)
    f = frames(o, 64, 32)[0]
    planes, st, _ = q.ctx.encode_frame(f, 1.0, 2)
    e, _, _ = orc.encode(f.copy(), 1.0, 2)
    assert all(np.array_equal(a, b) for a, b in zip(planes, e))
    assert same_bits(q.ctx.decode_frame(planes, st, 64, 32, 1.0, 2), orc.decode(e, st, 64, 32, 1.0, 2))
    # (b) 13-bit PQ table: threshold records in LDS (mode 3); the same table made non-monotone -> the reference's
    #     bisection on the global-memory table (mode 2)
    lut13 = L.build_lut(L.PTF_PQ, 13).copy()
    bad13 = lut13.copy()
    bad13[3000:3010] = bad13[3000:3010][::-1]
    #     lumahip_tune("lds_table_max_kb") moves the boundary: 64 -> records in global memory (mode 4), the decode kernels'
    #     32 KiB luminance table still in LDS; 0 -> the decode kernels read theirs from global memory as well
    for table, mode, kb in ((None, 3, None), (bad13, 2, None), (None, 4, 64), (None, 4, 0)):
        q2 = L.LumaQuantizer()
        if kb is not None:
            q2.ctx.tune("lds_table_max_kb", kb)
        q2.setQuantizer(L.PTF_PQ, 13, L.CS_XYZ, 8, 1e4, 0.005, mapping_override=table)
        assert q2.ctx.quantizer_info()["mode"] == mode
        orc2 = o.Oracle(o.PTF_PQ, 13, o.CS_XYZ, 8, 1e4, 0.005)
        if table is not None:
            orc2.overwrite_mapping(table)
        for profile in (2, 3):
            planes, st, _ = q2.ctx.encode_frame(f, 1.0, profile)
            e, _, _ = orc2.encode(f.copy(), 1.0, profile)
            assert all(np.array_equal(a, b) for a, b in zip(planes, e))
            assert same_bits(q2.ctx.decode_frame(planes, st, 64, 32, 1.0, profile), orc2.decode(e, st, 64, 32, 1.0, profile))
    # the shipped tables take the threshold-record path, in LDS
    for name in ("pq11_luv8", "log12_luv8", "pq12_rgb", "psi11_luv8"):
        q3 = L.LumaQuantizer()
        q3.setQuantizer(*CONFIGS[name])
        assert q3.ctx.quantizer_info()["mode"] == 3, name


def test_unaligned_strides_and_bad_arguments(L, oracle_mod):
    o = oracle_mod
    q, orc = pair(L, o, CONFIGS["pq11_luv8"])
    f = frames(o, 66, 34)[0]
    # odd strides force the byte-store path
    planes, st, _ = q.ctx.encode_frame(f, 1.0, 2, strides=(66 * 2 + 3, 33 * 2 + 1, 33 * 2 + 5))
    g = f.copy()
    orc.transform(g, True, 1.0)
    for p in range(3):
        w = 66 if p == 0 else 33
        h = 34 if p == 0 else 17
        ref = np.zeros((h, st[p]), dtype=np.uint8)
        orc.L.lo_pack_plane(__import__("ctypes").byref(orc.q), g[p].ctypes.data, p, 2, 66, 34, ref.ctypes.data, st[p], None)
        assert np.array_equal(planes[p][:, :2 * w], ref[:, :2 * w])
    with pytest.raises(L.LumaHipError):      # "Invalid frame size", src/luma_encoder.cpp:118-119
        q.ctx.encode_frame(np.zeros((3, 5, 8), dtype=np.float32), 1.0, 2)
    with pytest.raises(L.LumaHipError):
        q.ctx.encode_frame(np.zeros((3, 4, 8), dtype=np.float32), 1.0, 7)
    for empty in ((3, 0, 8), (3, 4, 0)):          # empty frames: "Invalid frame size" as well
        with pytest.raises(L.LumaHipError):
            q.ctx.encode_frame(np.zeros(empty, dtype=np.float32), 1.0, 2)
    assert q.transformColorSpace(np.zeros((3, 0, 0), dtype=np.float32), True, 1.0) is True   # zero iterations, true
    with pytest.raises(L.LumaHipError):           # no quantizer set yet
        L.Context().encode_frame(np.ones((3, 2, 2), dtype=np.float32))
    bad = L.LumaQuantizer()
    bad.setQuantizer(L.PTF_PQ, 11, 9, 8, 1e4, 0.005)   # unknown colour space: transformColorSpace returns false
    assert bad.transformColorSpace(np.ones((3, 2, 2), dtype=np.float32), True, 1.0) is False
    # device entry points: layouts in which rows / frames would overlap or fall outside a plane are refused
    import torch
    dev = torch.device("cuda:0")
    w, h, n3 = 64, 32, 3 * 64 * 32
    src = torch.zeros(2 * n3, dtype=torch.float32, device=dev)
    out = torch.zeros(2 * n3, dtype=torch.float32, device=dev)
    pl = [torch.zeros(2 * 32 * 128, dtype=torch.uint8, device=dev) for _ in range(3)]
    ptr = [t.data_ptr() for t in pl]
    ok_st, ok_pfs = (128, 64, 64), (32 * 128, 16 * 64, 16 * 64)
    q.ctx.encode_frames_device(src.data_ptr(), n3, 2, w, h, 1.0, 2, ptr, ok_st, ok_pfs)           # the valid layout
    q.ctx.decode_frames_device(ptr, ok_st, ok_pfs, 2, w, h, 2, 1.0, out.data_ptr(), n3)
    for st_, pfs_, fs_ in (((126, 64, 64), ok_pfs, n3), ((128, 62, 64), ok_pfs, n3), ((-128, 64, 64), ok_pfs, n3),
                           (ok_st, (0, 0, 0), n3), (ok_st, (32 * 128 - 2, 16 * 64, 16 * 64), n3), (ok_st, ok_pfs, n3 - 2),
                           (ok_st, ok_pfs, 0)):
        with pytest.raises(L.LumaHipError):
            q.ctx.encode_frames_device(src.data_ptr(), fs_, 2, w, h, 1.0, 2, ptr, st_, pfs_)
        with pytest.raises(L.LumaHipError):
            q.ctx.decode_frames_device(ptr, st_, pfs_, 2, w, h, 2, 1.0, out.data_ptr(), fs_)
    torch.cuda.synchronize()


@pytest.mark.parametrize("do_tmo,ldr_sim,exposure,gamma", [(0, 0, 1.0, 2.2), (1, 0, 0.02, 2.2), (0, 1, 1.0, 1.8), (1, 1, 4.0, 2.4)])
def test_decode_display_transform(L, oracle_mod, do_tmo, ldr_sim, exposure, gamma):
    """decode fused with the player's display transform (src/lumaplay_dequantizer.frag:145-156): RGBA8 within
    +-1 code of a float64 evaluation on the (bit-exact) decoded floats; the float output, when also requested,
    stays bit-exact."""
    import torch
    o = oracle_mod
    w, h = 256, 64
    q, orc = pair(L, o, CONFIGS["pq11_luv8"])
    f = o.synth_frame(w, h, frame=11) * np.float32(0.01)
    planes, st, _ = orc.encode(f.copy(), 1.0, 2)
    dec = orc.decode(planes, st, w, h, 1.0, 2)
    dev = torch.device("cuda:0")
    tp = [torch.from_numpy(p.copy()).to(dev) for p in planes]
    rgba = torch.zeros(h * w * 4, dtype=torch.uint8, device=dev)
    rgb = torch.zeros(3 * h * w, dtype=torch.float32, device=dev)
    q.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    q.ctx.decode_display_frames_device([t.data_ptr() for t in tp], st, [0, 0, 0], 1, w, h, 2, 1.0, rgba.data_ptr(), 4 * w, 0,
                                       exposure, gamma, do_tmo, ldr_sim, rgb_ptr=rgb.data_ptr(), frame_stride=3 * w * h)
    torch.cuda.synchronize()
    q.ctx.set_stream(None)
    assert same_bits(rgb.cpu().numpy().reshape(3, h, w), dec)
    exp = o.display_transform(dec.astype(np.float32), exposure, gamma, do_tmo, ldr_sim).astype(np.int32)     # oracle/luma_oracle.c lo_display_transform
    got = rgba.cpu().numpy().reshape(h, w, 4).astype(np.int32)
    assert np.all(got[..., 3] == 255)
    assert np.all(exp[..., 3] == 255)
    assert np.max(np.abs(got[..., :3] - exp[..., :3])) <= 1
    assert np.mean(got[..., :3] == exp[..., :3]) > 0.98
    # ... and a code differs only next to a rounding boundary, towards it (tests/support/display.py)
    t = display_t(dec, exposure, gamma, do_tmo, ldr_sim)
    assert np.array_equal(display_bytes(t), exp)
    check_rgba(rgba.cpu().numpy().reshape(h, w, 4), t, (do_tmo, ldr_sim, exposure, gamma))


def test_python_host_mirror_of_the_reference_interface(L, oracle_mod):
    """lumahdrv_amd.LumaFrameCodec / LumaQuantizer (the Python mirror of LumaEncoder::encode, LumaDecoder::decode and
    LumaQuantizer): defaults of the reference's parameter structs, profile adjustment, pack-only / unpack-only
    (setChannels / getVpxChannels on their own), decoder-style mapping override."""
    o = oracle_mod
    p = L.LumaEncoderParams()
    assert (p.ptfBitDepth, p.colorBitDepth, p.preScaling, p.profile, p.bitDepth, p.ptf, p.colorSpace) == (11, 8, 1.0, 2, 12, L.PTF_PQ, L.CS_LUV)
    assert L.LumaDecoderParams().ptf == L.PTF_PSI           # include/luma/luma_decoder.h:62
    codec = L.LumaFrameCodec(p)
    orc = o.Oracle(o.PTF_PQ, 11, o.CS_LUV, 8, 1e4, 0.005)
    f = o.test_frame(128, 64)
    planes, st, mean = codec.encode(f)
    e, _, avg = orc.encode(f.copy(), 1.0, 2)
    assert all(np.array_equal(a, b) for a, b in zip(planes, e)) and mean == pytest.approx(avg, rel=1e-3)
    assert same_bits(codec.decode(planes, st, 128, 64), orc.decode(e, st, 128, 64, 1.0, 2))
    # bitDepth 8 moves profile 2 -> 0 (src/luma_encoder.cpp:68-72)
    p8 = L.LumaEncoderParams(bitDepth=8, ptfBitDepth=8)
    c8 = L.LumaFrameCodec(p8)
    assert c8.params.profile == 0
    pl8, st8, _ = c8.encode(f)
    e8, _, _ = o.Oracle(o.PTF_PQ, 8, o.CS_LUV, 8, 1e4, 0.005).encode(f.copy(), 1.0, 0)
    assert all(np.array_equal(a, b) for a, b in zip(pl8, e8))
    # setChannels / getVpxChannels on their own == the oracle's pack / unpack of an already transformed frame
    q = codec.quant
    g = f.copy()
    assert q.transformColorSpace(g, True, 1.0)
    packed, pst, _ = q.ctx.pack_frame(g, 2)
    assert all(np.array_equal(a, b) for a, b in zip(packed, e))
    un = q.ctx.unpack_frame(packed, pst, 128, 64, 2)
    exp = np.empty_like(un)
    import ctypes as C
    for pl in range(3):
        orc.L.lo_unpack_plane(C.byref(orc.q), e[pl].ctypes.data, st[pl], pl, 2, 128, 64, exp[pl].ctypes.data)
    assert same_bits(un, exp)
    assert q.getSize() == 2047 and q.getMapping().size == 2048 and q.getMaxLum() == 1e4
    # decoder-style override: attachment 434 carries getSize() floats, the last entry stays this side's
    q2 = L.LumaQuantizer()
    ov = (q.getMapping()[:-1] * np.float32(1.5)).astype(np.float32)
    q2.setQuantizer(L.PTF_PQ, 11, L.CS_LUV, 8, 1e4, 0.005, mapping_override=ov)
    assert q2.getMapping()[-1] == q.getMapping()[-1] and q2.getMapping()[5] == ov[5]


def test_pipelined_batch_host_entry_points(L, oracle_mod):
    """lumahip_encode_frames_host / lumahip_decode_frames_host (3-slot pipeline over three streams) give exactly
    the results of single-frame calls, for more frames than slots and with pinned and pageable buffers"""
    o = oracle_mod
    q, orc = pair(L, o, CONFIGS["pq11_luv8"])
    w, h, n = 320, 180, 8
    frames = [o.synth_frame(w, h, frame=100 + i) for i in range(n)]
    q.ctx.host_register(frames[0])
    try:
        planes, st, means = q.ctx.encode_frames(frames, 1.0, 2)
    finally:
        q.ctx.host_unregister(frames[0])
    for i in range(n):
        e, _, avg = orc.encode(frames[i].copy(), 1.0, 2)
        assert all(np.array_equal(a, b) for a, b in zip(planes[i], e)), i
        assert means[i] == pytest.approx(avg, rel=1e-3)
    outs = q.ctx.decode_frames(planes, st, w, h, 1.0, 2)
    for i in range(n):
        assert same_bits(outs[i], orc.decode(planes[i], st, w, h, 1.0, 2)), i
    # a second batch of a different size re-sizes the slots
    f2 = [o.synth_frame(64, 32, frame=i) for i in range(4)]
    p2, st2, _ = q.ctx.encode_frames(f2, 1.0, 3)
    for i in range(4):
        e, _, _ = orc.encode(f2[i].copy(), 1.0, 3)
        assert all(np.array_equal(a, b) for a, b in zip(p2[i], e))


def test_pageable_buffers_are_staged_in_chunks_with_padded_strides(L, oracle_mod):
    """Pageable caller memory moves through 8 MiB pinned chunks (lumahip_host.hip: xfer_h2d_2d / xfer_d2h_2d).  A 4K
    frame with row strides wider than the rows makes every plane a multi-chunk, row-by-row transfer in both directions;
    results equal the oracle's and the padding bytes of the caller's planes are never written."""
    o = oracle_mod
    q, orc = pair(L, o, CONFIGS["pq11_luv8"])
    w, h = 3840, 2160
    f = o.synth_frame(w, h, frame=21)
    strides = (2 * w + 96, w + 32, w + 32)
    planes, st, _ = q.ctx.encode_frame(f, 1.0, 2, strides=strides)
    assert tuple(st) == strides
    e, est, _ = orc.encode(f.copy(), 1.0, 2, threads=8)
    rb = (2 * w, w, w)
    for p in range(3):
        ep = o.packed_rows(e[p], rb[p])
        assert np.array_equal(planes[p][:, :rb[p]].reshape(-1), np.asarray(ep).reshape(-1)), p
        assert not planes[p][:, rb[p]:].any(), p   # padding untouched (the buffers start zeroed)
    got = q.ctx.decode_frame(planes, st, w, h, 1.0, 2)
    assert same_bits(got, orc.decode(e, est, w, h, 1.0, 2, threads=8))


@pytest.mark.parametrize("rgb,codes", [
    ((1, 1, 1), (307, 81, 192)), ((100, 100, 100), (1040, 81, 192)), ((10000, 0, 0), (1707, 185, 214)),
    ((0, 10000, 0), (1975, 51, 231)), ((0, 0, 10000), (1466, 72, 65)), ((0, 0, 0), (3, 86, 194)),
    ((1e-6, 1e-6, 1e-6), (3, 86, 194)), ((0.5, 20, 3), (676, 53, 222)), ((-5, 2, 1), (229, 0, 164)),
    ((np.nan, 1, 1), (2047, 255, 255)), ((np.inf, 1, 1), (2047, 86, 194)), ((65504, 65504, 65504), (2047, 81, 192)),
])
def test_survey_constant_colour_pins_on_gpu(L, rgb, codes):
    """the known-answer codes SURVEY.md 8(c) recorded from the real reference encoder, straight through the C ABI"""
    q = L.LumaQuantizer()
    q.setQuantizer(*CONFIGS["pq11_luv8"])
    f = np.empty((3, 2, 2), dtype=np.float32)
    for c in range(3):
        f[c] = np.float32(rgb[c])
    planes, _, _ = q.ctx.encode_frame(f, 1.0, 2)
    got = (int(planes[0].view("<u2")[0, 0]), int(planes[1].view("<u2")[0, 0]), int(planes[2].view("<u2")[0, 0]))
    assert got == codes
    assert np.all(planes[0].view("<u2")[:2, :2] == codes[0])


@pytest.mark.parametrize("rgb,codes", [
    ((1, 1, 1), (573, 514, 514)), ((0.5, 20, 3), (755, 470, 344)), ((0, 0, 0), (64, 514, 514)),
    ((10000, 0, 0), (403, 329, 1023)), ((np.nan, 1, 1), (1023, 1023, 1023)),
])
def test_survey_ycbcr_pins_on_gpu(L, rgb, codes):
    q = L.LumaQuantizer()
    q.setQuantizer(*CONFIGS["pq10_ycbcr10"])
    f = np.empty((3, 2, 2), dtype=np.float32)
    for c in range(3):
        f[c] = np.float32(rgb[c])
    planes, _, _ = q.ctx.encode_frame(f, 20.0, 2)
    assert (int(planes[0].view("<u2")[0, 0]), int(planes[1].view("<u2")[0, 0]), int(planes[2].view("<u2")[0, 0])) == codes


@pytest.mark.parametrize("profile", [0, 1, 2, 3])
def test_kernels_write_only_inside_their_planes(L, oracle_mod, profile):
    """guard bands around every device buffer and the stride padding of every row must come back untouched, for
    sizes that leave partially filled tiles (the unit / tile grid overhangs the frame)"""
    import torch
    o = oracle_mod
    cfg = CONFIGS["pq8_luv8"] if profile < 2 else CONFIGS["pq11_luv8"]
    q, orc = pair(L, o, cfg)
    dev = torch.device("cuda:0")
    G = 4096
    q.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    for (w, h, nf) in ((258, 10, 3), (64, 6, 2), (1284, 22, 1)):
        n3 = 3 * w * h
        _, hs, st, bps = L.plane_geometry(w, h, profile)
        st = tuple(s + 16 for s in st)                      # extra stride padding that must stay untouched
        ws = (w, w // 2 if profile in (0, 2) else w, w // 2 if profile in (0, 2) else w)
        psz = [hs[p] * st[p] for p in range(3)]
        frames = np.stack([o.synth_frame(w, h, frame=7 + i) for i in range(nf)])
        src = torch.from_numpy(frames.reshape(-1)).to(dev)
        bufs = [torch.full((G + nf * psz[p] + G,), 0xA5, dtype=torch.uint8, device=dev) for p in range(3)]
        q.ctx.encode_frames_device(src.data_ptr(), n3, nf, w, h, 1.0, profile, [b.data_ptr() + G for b in bufs], st, psz)
        torch.cuda.synchronize()
        for p in range(3):
            hb = bufs[p].cpu().numpy()
            assert np.all(hb[:G] == 0xA5) and np.all(hb[-G:] == 0xA5), (w, h, p)
            body = hb[G:-G].reshape(nf, hs[p], st[p])
            assert np.all(body[:, :, ws[p] * bps:] == 0xA5), (w, h, p)
            for i in range(nf):
                e, _, _ = orc.encode(frames[i].copy(), 1.0, profile)
                assert np.array_equal(body[i][:, :ws[p] * bps], e[p][:, :ws[p] * bps]), (w, h, p, i)
        out = torch.full((G // 4 + nf * n3 + G // 4,), -777.0, dtype=torch.float32, device=dev)
        q.ctx.decode_frames_device([b.data_ptr() + G for b in bufs], st, psz, nf, w, h, profile, 1.0,
                                   out.data_ptr() + G, n3)
        torch.cuda.synchronize()
        ho = out.cpu().numpy()
        assert np.all(ho[:G // 4] == -777.0) and np.all(ho[-(G // 4):] == -777.0)
        assert np.all(np.isfinite(ho[G // 4:-(G // 4)]))
    q.ctx.set_stream(None)


def test_per_frame_statistics_exact_min_max(L, oracle_mod):
    """the optional per-frame statistics of the encode kernel (wave64 reductions + float atomics): min and max of
    transformed channel 0 are order-independent, so they must equal the oracle's exactly; the sum (the reference's
    mean-luminance accumulator, src/luma_encoder.cpp:276,294,314) to float tolerance.  Several frames per launch,
    tiles overhanging the frame."""
    import torch
    o = oracle_mod
    dev = torch.device("cuda:0")
    for name in ("pq11_luv8", "pq12_rgb", "pq10_ycbcr10"):
        cfg = CONFIGS[name]
        q, orc = pair(L, o, cfg)
        q.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        w, h, nf = 1284, 70, 5
        n3 = 3 * w * h
        frames = np.stack([o.synth_frame(w, h, frame=40 + i) * np.float32(1 + i) for i in range(nf)])
        src = torch.from_numpy(frames.reshape(-1)).to(dev)
        _, hs, st, _ = L.plane_geometry(w, h, 2)
        psz = [hs[p] * st[p] for p in range(3)]
        planes = [torch.zeros(nf * psz[p], dtype=torch.uint8, device=dev) for p in range(3)]
        stats = torch.zeros(3 * nf, dtype=torch.float32, device=dev)
        q.ctx.encode_frames_device(src.data_ptr(), n3, nf, w, h, 1.0, 2, [p.data_ptr() for p in planes], st, psz,
                                   stats.data_ptr())
        torch.cuda.synchronize()
        s = stats.cpu().numpy().reshape(nf, 3)
        for i in range(nf):
            t = frames[i].copy()
            orc.transform(t, True, 1.0)
            assert s[i, 1] == t[0].min() and s[i, 2] == t[0].max(), (name, i)
            assert s[i, 0] == pytest.approx(float(t[0].astype(np.float64).sum()), rel=1e-4)
        q.ctx.set_stream(None)


def test_planes_match_the_reference_loops_fixtures(L, golden_dir):
    """The HIP path straight against tests/golden/ref_planes.npz -- outputs of the reference's OWN compiled
    LumaEncoder::setChannels (after transformColorSpace) and LumaDecoder::getVpxChannels (+ inverse transform), no oracle
    in between: 4 configurations x the profiles their bit depth allows x 2 sizes; decode side with decoder-chosen odd
    strides and out-of-range codes.  Planes bit-exact, floats 0 ulp."""
    gp = np.load(os.path.join(golden_dir, "ref_planes.npz"))
    keys = sorted(k[:-3] for k in gp.files if k.endswith("_in"))
    assert len(keys) == 16
    for key in keys:
        name, size, prof = key.rsplit("_", 2)
        cfg = CONFIGS[name]
        w, h = (int(x) for x in size.split("x"))
        profile = int(prof[1])
        sc = 20.0 if cfg[2] == L.CS_YCBCR else 1.0
        q = L.LumaQuantizer()
        q.setQuantizer(*cfg)
        planes, st, mean = q.ctx.encode_frame(gp[key + "_in"].copy(), sc, profile)
        assert tuple(st) == tuple(gp[key + "_stride"])
        sub, bps = profile in (0, 2), (2 if profile > 1 else 1)
        rb = (w * bps, ((w + 1) // 2 if sub else w) * bps, ((w + 1) // 2 if sub else w) * bps)
        for p in range(3):
            assert np.array_equal(planes[p][:, :rb[p]], gp[key + "_plane%d" % p][:, :rb[p]]), (key, p)
        dst = tuple(int(x) for x in gp[key + "_dec_stride"])
        dpl = [gp[key + "_dec_plane%d" % p] for p in range(3)]
        assert same_bits(q.ctx.unpack_frame(dpl, dst, w, h, profile), gp[key + "_unpacked"]), key
        assert same_bits(q.ctx.decode_frame(dpl, dst, w, h, sc, profile), gp[key + "_decoded"]), key


def test_reference_loop_digests_on_gpu(L, oracle_mod, golden_dir):
    """testFrame 1280x720 encode -> decode on the GPU reproduces the digests recorded from the reference's own loops
    (tests/golden/ref_plane_digests.json): Y/U/V for profiles 2 and 3 and the decoded frame."""
    import json
    o = oracle_mod
    dig = json.load(open(os.path.join(golden_dir, "ref_plane_digests.json")))
    q = L.LumaQuantizer()
    q.setQuantizer(*CONFIGS["pq11_luv8"])
    for profile in (2, 3):
        d = dig["testframe_1280x720_p%d" % profile]
        planes, st, _ = q.ctx.encode_frame(o.test_frame(1280, 720), 1.0, profile)
        cb = 2560 if profile == 3 else 1280
        assert (o.survey_digest(o.packed_rows(planes[0], 2560)), o.survey_digest(o.packed_rows(planes[1], cb)),
                o.survey_digest(o.packed_rows(planes[2], cb))) == (d["Y"], d["U"], d["V"])
        assert o.survey_digest(q.ctx.decode_frame(planes, st, 1280, 720, 1.0, profile)) == d["decoded"]


@pytest.mark.parametrize("w,h", [(1920, 1080), (3840, 2160)])
def test_mean_luminance_against_the_references_sequential_sum(L, oracle_mod, w, h):
    """LumaEncoder::setVpxChannel sums plane 0 sequentially in fp32 (src/luma_encoder.cpp:276,294,314) -- a sum that
    drops small addends once it is large.  At full size: (a) the kernels' statistic is the ACCURATE mean (1e-5 of a
    float64 sum) and therefore differs from the reference's number (documented in INTEGRATION.md); (b)
    lumahip_mean_luminance_reference_device reproduces the reference's sequential sum bit for bit; (c) frames whose mean
    lies anywhere near the warning threshold get that exact value from the host entry points, so the `avg <= 1`
    decision is the reference's even where the two sums disagree."""
    import torch
    o = oracle_mod
    q, orc = pair(L, o, CONFIGS["pq11_luv8"])
    f = o.synth_frame(w, h, frame=3)
    g64 = f.copy()
    orc.transform(g64, True, 1.0)
    true_mean = float(g64[0].astype(np.float64).mean())
    _, _, seq = orc.encode(f.copy(), 1.0, 2, threads=1)             # the reference's order
    _, _, fast = q.ctx.encode_frame(f, 1.0, 2)
    assert abs(fast - true_mean) <= 1e-5 * true_mean
    assert abs(seq - true_mean) > 1e-4 * true_mean                  # the reference's own sum is the inaccurate one
    d = torch.from_numpy(f).cuda()
    exact = q.ctx.mean_luminance_reference_device(d.data_ptr(), w, h, 1.0)
    assert np.float32(exact) == np.float32(seq)
    # frames around the threshold: accurate mean 0.9 ... 1.3; the sequential sum may land on the other side of 1.0
    sides = set()
    for target in (0.9, 0.99995, 1.00005, 1.05, 1.3):
        g = (f * np.float32(target / true_mean)).astype(np.float32)
        _, _, seq_g = orc.encode(g.copy(), 1.0, 2, threads=1)
        _, _, host = q.ctx.encode_frame(g, 1.0, 2)
        assert np.float32(host) == np.float32(seq_g)                  # exact, hence the same `avg <= 1.0f` decision
        sides.add((target > 1.0, seq_g > 1.0))
        if target in (0.99995, 1.05):
            _, _, host_b = q.ctx.encode_frames([g, f], 1.0, 2)        # the pipelined batch entry point too
            assert np.float32(host_b[0]) == np.float32(seq_g) and abs(host_b[1] - true_mean) <= 1e-5 * true_mean
            qf = L.LumaQuantizer()
            qf.setQuantizer(*CONFIGS["pq11_luv8"])
            _, _, host_t, _ = qf.ctx.encode_frame(g, 1.0, 2, want_transformed=True)   # the facade's call shape
            assert np.float32(host_t) == np.float32(seq_g)
    assert len(sides) >= 2


def test_fast_division_forms_equal_ieee_division_build(L, oracle_mod, tmp_path):
    """The kernels use shortened division sequences where operand ranges license them (div_nr / div_255_pos / div_219_fin,
    luma_device.hpp).  A second build of the same library with -DLH_NO_FAST_DIV (every division through the compiler's
    full IEEE sequence; lumahdrv_amd/lib_nofastdiv, built by __graft_entry__.build()) must produce identical planes and
    floats on inputs chosen to sit on the range edges: X, Y, Z at / beyond the 1e-4 and 1e8 clamps in every mix, zero /
    huge / non-finite components, chroma codes 0, 1, maxC, out of range, luminance codes at the table ends, PQ peaks
    Lmax = 1e-6 and 1e9 for the YCbCr path."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    alt = os.path.join(root, "lumahdrv_amd", "lib_nofastdiv", "liblumahip.so")
    if not os.path.exists(alt):
        from lumahdrv_amd import capi
        capi.build_library(nofastdiv=True)
    vals = np.array([0, 1e-7, 1e-4, 3e-4, 1, 97.0, 1e4, 9e7, 1e8, 4e8, 1e12, 8e37, np.inf, np.nan, -1.0], dtype=np.float32)
    r, g, b = np.meshgrid(vals, vals, vals, indexing="ij")
    edge = np.stack([r.ravel(), g.ravel(), b.ravel()])                 # 3375 pixels
    n = edge.shape[1] + (-edge.shape[1]) % 64
    frame = np.ones((3, n), dtype=np.float32)
    frame[:, :edge.shape[1]] = edge
    frame = frame.reshape(3, -1, 64)[:, : (frame.size // 3 // 64) // 2 * 2].copy()   # even height
    rng = np.random.default_rng(9)
    wide = np.exp(rng.uniform(np.log(1e-9), np.log(1e10), size=(3, 64, 64))).astype(np.float32)
    np.savez(tmp_path / "in.npz", edge=frame, wide=wide)
    worker = r"""
import sys, numpy as np
sys.path.insert(0, %r)
import lumahdrv_amd as L
d = np.load(sys.argv[1])
out = {}
cfgs = {"luv": (1, 11, 0, 8, 1e4, 0.005), "xyz": (4, 12, 3, 8, 1e4, 0.005), "rgb": (1, 12, 1, 8, 1e4, 0.005),
        "ycc": (1, 10, 2, 10, 1000.0, 0.01), "ycc_lo": (1, 10, 2, 10, 1e-6, 0.01), "ycc_hi": (1, 10, 2, 10, 1e9, 0.01)}
for name, cfg in cfgs.items():
    q = L.LumaQuantizer(); q.setQuantizer(*cfg)
    for fname in ("edge", "wide"):
        f = d[fname]
        hh, ww = f.shape[1:]
        for sc in (1.0, 20.0, 0.25):
            for profile in (2, 3):
                planes, st, _ = q.ctx.encode_frame(f, sc, profile)
                for p in range(3):
                    out["%%s_%%s_%%g_%%d_p%%d" %% (name, fname, sc, profile, p)] = planes[p]
                # decode what was encoded, plus every code combination at the range edges
                out["%%s_%%s_%%g_%%d_dec" %% (name, fname, sc, profile)] = q.ctx.decode_frame(planes, st, ww, hh, sc, profile)
    maxv, maxc = 2 ** cfg[1] - 1, 2 ** cfg[3] - 1
    lum = np.array([0, 1, maxv // 2, maxv - 1, maxv, maxv + 1, 65535], dtype=np.uint16)
    chr_ = np.array([0, 1, maxc // 2, maxc - 1, maxc, maxc + 1, 65535], dtype=np.uint16)
    a, bb, cc = np.meshgrid(lum, chr_, chr_, indexing="ij")
    codes = [x.ravel() for x in (a, bb, cc)]
    npx = codes[0].size + (-codes[0].size) %% 16
    pl = []
    for x in codes:
        y = np.zeros(npx, dtype="<u2"); y[:x.size] = x
        pl.append(y.reshape(-1, 8).view(np.uint8).copy())
    hh, ww = pl[0].shape[0], 8
    hh -= hh %% 2
    pl = [p_[:hh] for p_ in pl]
    for sc in (1.0, 20.0):
        out["%%s_codes_%%g" %% (name, sc)] = q.ctx.decode_frame(pl, (16, 16, 16), ww, hh, sc, 3)
np.savez(sys.argv[2], **out)
from lumahdrv_amd import capi
print("LIB", capi.library_path())
""" % (root,)
    outs = {}
    for tag, lib in (("fast", None), ("ieee", alt)):
        env = dict(os.environ)
        if lib:
            env["LUMAHIP_LIB"] = lib
        else:
            env.pop("LUMAHIP_LIB", None)
        p = subprocess.run([sys.executable, "-c", worker, str(tmp_path / "in.npz"), str(tmp_path / (tag + ".npz"))],
                           capture_output=True, text=True, env=env, timeout=900)
        assert p.returncode == 0, p.stderr[-3000:]
        assert ("lib_nofastdiv" in p.stdout) == (lib is not None), p.stdout       # the build that was asked for was loaded
        outs[tag] = np.load(tmp_path / (tag + ".npz"))
    assert set(outs["fast"].files) == set(outs["ieee"].files) and len(outs["fast"].files) >= 300
    for k in outs["fast"].files:
        a, b_ = outs["fast"][k], outs["ieee"][k]
        if a.dtype == np.float32:
            assert same_bits(a, b_), k
        else:
            assert np.array_equal(a, b_), k


def test_random_monotone_tables_through_the_encode_kernel(L, oracle_mod):
    """Arbitrary attachment-434 style tables (random non-decreasing, 10- and 12-bit, log-uniform over 60 decades / linear /
    with a duplicate) through k_encode<CS_RGB, 4:4:4> with whatever search the library picks (records in LDS or global
    memory, or the literal bisection when the builder refuses the table), on every table entry's neighbourhood and the
    midpoints' rounding-tie zone: planes bit-exact against the oracle's literal search."""
    o = oracle_mod
    rng = np.random.default_rng(77)
    modes = set()
    for trial in range(12):
        bits = 10 if trial % 2 else 12
        n = 1 << bits
        if trial % 3 == 0:
            m = np.sort(np.exp(rng.uniform(np.log(1e-30), np.log(1e30), n))).astype(np.float32)
        elif trial % 3 == 1:
            m = np.sort(rng.uniform(0, 1e4, n)).astype(np.float32)
        else:
            m = np.sort(np.exp(rng.uniform(np.log(1e-3), np.log(1e5), n))).astype(np.float32)
            m[n // 2 + 1] = m[n // 2]
            if trial == 8:
                m[7:10] = m[7]                      # a triple: the record builder refuses, literal kernels take over
        q = L.LumaQuantizer()
        q.setQuantizer(L.PTF_PQ, bits, L.CS_RGB, 8, 1e4, 0.005, mapping_override=m)
        modes.add(q.ctx.quantizer_info()["mode"])
        orc = o.Oracle(o.PTF_PQ, bits, o.CS_RGB, 8, 1e4, 0.005)
        orc.overwrite_mapping(m)
        mids = ((m[:-1].astype(np.float64) + m[1:]) / 2).astype(np.float32)
        v = np.concatenate([m, np.nextafter(m, np.float32(np.inf)), np.nextafter(m, np.float32(-np.inf)), mids,
                            np.nextafter(mids, np.float32(np.inf)), np.nextafter(mids, np.float32(-np.inf)),
                            np.array([0.0, -0.0, -1.0, np.inf, -np.inf, np.nan, 1e-45, 3.4e38], dtype=np.float32)])
        v = np.concatenate([v, np.ones((-v.size) % 8, dtype=np.float32)])
        frame = np.stack([v.reshape(2, -1), v[::-1].reshape(2, -1), np.roll(v, 3).reshape(2, -1)]).copy()
        planes, st, _ = q.ctx.encode_frame(frame, 1.0, 3)
        exp, _, _ = orc.encode(frame.copy(), 1.0, 3)
        for p in range(3):
            assert np.array_equal(planes[p], exp[p]), (trial, p)
    assert 0 in modes and (3 in modes or 4 in modes)


@pytest.mark.parametrize("name,nframes", [("pq11_luv8", 8), ("log12_luv8", 8), ("pq10_ycbcr10", 20)])
def test_long_batched_launches_are_bit_exact(L, oracle_mod, name, nframes):
    """Batched launches long enough for the launch-geometry rules of lumahip_launch.hip: grid_for / block_threads_for (3
    workgroups per CU for the 256-thread encode kernels, 256-thread workgroups for LOG-12, 5 per CU for the 4:2:0 16-bit
    decode kernels, 18 / 12 static shares per CU for YCbCr) -- every frame of the batch against the oracle, planes and
    decoded floats, bit for bit."""
    import torch
    o = oracle_mod
    cfg = CONFIGS[name]
    q, orc = pair(L, o, cfg)
    w, h, profile = 3840, 2160, 2
    sc = 20.0 if cfg[2] == o.CS_YCBCR else 1.0
    n3 = 3 * w * h
    dev = torch.device("cuda:0")
    _, hs, st, _ = L.plane_geometry(w, h, profile)
    psz = [hs[p] * st[p] for p in range(3)]
    src = torch.empty(nframes * n3, dtype=torch.float32, device=dev)
    out = torch.empty(nframes * n3, dtype=torch.float32, device=dev)
    planes = [torch.zeros(nframes * psz[p], dtype=torch.uint8, device=dev) for p in range(3)]
    q.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    q.ctx.synth_frames_device(src.data_ptr(), n3, nframes, w, h, 4242, 0)
    pl = [p.data_ptr() for p in planes]
    q.ctx.encode_frames_device(src.data_ptr(), n3, nframes, w, h, sc, profile, pl, st, psz)
    q.ctx.decode_frames_device(pl, st, psz, nframes, w, h, profile, sc, out.data_ptr(), n3)
    torch.cuda.synchronize()
    q.ctx.set_stream(None)
    nt = os.cpu_count() or 1
    for f in range(nframes):
        frame = o.synth_frame(w, h, 4242, f)
        e, est, _ = orc.encode(frame.copy(), sc, profile, threads=nt)
        for p in range(3):
            got = planes[p][f * psz[p]:(f + 1) * psz[p]].cpu().numpy().reshape(hs[p], st[p])
            assert np.array_equal(got, e[p]), (name, f, p)
        exp = orc.decode(e, est, w, h, sc, profile, threads=nt)
        assert same_bits(out[f * n3:(f + 1) * n3].cpu().numpy().reshape(3, h, w), exp), (name, f)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_extreme_inputs_bit_exact(L, oracle_mod, name):
    """inf - inf patterns inside the RGB -> XYZ rows, +-FLT_MAX, NaNs of both signs in every position, -0, denormals
    (tests/golden/make_golden.py: extreme_frame; the oracle is pinned on exactly this frame against the live reference by
    tests/test_oracle_golden.py): planes of every profile and the forward transform, bit for bit.  This is the frame that
    would expose a clamp that treats NaN or infinity differently from std::max(std::min(v, 1e8f), 1e-4f)."""
    o = oracle_mod
    cfg = CONFIGS[name]
    q, orc = pair(L, o, cfg)
    f = extreme_frame()
    for sc in (1.0, 20.0):
        a, b = f.copy(), f.copy()
        assert q.transformColorSpace(a, True, sc)
        with np.errstate(all="ignore"):
            orc.transform(b, True, sc)
        assert same_bits(a, b), (name, sc)
        for profile in (0, 1, 2, 3):
            planes, st, _ = q.ctx.encode_frame(f.copy(), sc, profile)
            with np.errstate(all="ignore"):
                e, _, _ = orc.encode(f.copy(), sc, profile)
            for p in range(3):
                assert np.array_equal(planes[p], e[p]), (name, sc, profile, p)
