"""Binary16 frames on the device (include/lumahip.h, lumahip_*_f16).

1. Against the reference's own output: decoding the _dec_plane* planes of tests/golden/ref_planes.npz through the host and the
   device f16 calls gives floatToHalf(_decoded) bit for bit -- what the reference's lumadec writes into its EXR.
2. f16 decode == the narrowed float decode of the same call: the parity configurations, profiles 0-3, ragged sizes, packed and
   planar layouts, batches, random (out-of-range) codes; inf, NaN and denormal results occur.
3. f16 encode == the float encode of the widened frame (planes and statistics) == the oracle: every search mode (literal LDS /
   global, records LDS / global, value-keyed), YCbCr at sc 1 and 20 with and without statistics and at a (sc, maxLum) without a
   half-input table, widths 258 / 34 / 6, profiles 0-3.
4. Full size: a 4K PQ-11 Lu'v' batch of 8 frames and a 4K HDR10 frame, both ways.
5. The device narrowing equals floatToHalf for all 2^32 floats.
6. torch.float16 tensors as device buffers in both directions.
7. Argument errors.
"""
import numpy as np
import pytest

from tests.golden.make_golden import CONFIGS
from tests.support.device import L, ctx, dev  # noqa: F401  (L is the module fixture)
from tests.support.host import float_to_half_np, widen_halves as _widen

pytestmark = pytest.mark.gpu


def _tensor_u8(arrs):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a).ravel()).to(dev()) for a in arrs]


def _sc_for(cfg):
    return 20.0 if cfg[2] == 2 else 1.0


# ---- 1. the reference's own decoded frames, narrowed as its EXR writer narrows them
def test_decode_f16_equals_reference_lumadec_halves(L, golden_dir):
    import os
    import torch
    gp = np.load(os.path.join(golden_dir, "ref_planes.npz"))
    keys = sorted(k[:-3] for k in gp.files if k.endswith("_in"))
    assert len(keys) == 16
    for key in keys:
        name, size, prof = key.rsplit("_", 2)
        cfg = CONFIGS[name]
        w, h = (int(x) for x in size.split("x"))
        profile = int(prof[1])
        sc = _sc_for(cfg)
        c = ctx(L, cfg)
        dst = tuple(int(x) for x in gp[key + "_dec_stride"])
        dpl = [gp[key + "_dec_plane%d" % p] for p in range(3)]
        exp = float_to_half_np(gp[key + "_decoded"])
        got = c.decode_frame_f16(dpl, dst, w, h, sc, profile)
        assert got.dtype == np.float16 and np.array_equal(got.view(np.uint16), exp), key
        tp = _tensor_u8(dpl)
        out = torch.empty(3 * h * w, dtype=torch.float16, device=dev())
        c.decode_frames_device_f16([t.data_ptr() for t in tp], dst, [t.numel() for t in tp], 1, w, h, profile, sc,
                                   out.data_ptr(), 3 * h * w)
        c.sync()
        assert np.array_equal(out.cpu().numpy().view(np.uint16), exp.ravel()), key


# ---- 2. f16 decode vs the narrowed float decode
def _random_buffers(rng, w, h, profile, nframes):
    _, hs, st, bps = L_geometry(w, h, profile)
    return [rng.integers(0, 256, size=nframes * hs[p] * st[p], dtype=np.uint8) for p in range(3)], st, \
        [hs[p] * st[p] for p in range(3)]


def L_geometry(w, h, profile):
    from lumahdrv_amd import plane_geometry
    return plane_geometry(w, h, profile)


DEC_SIZES = [(34, 18), (258, 6), (64, 32), (6, 4)]
# + a table deeper than 12 bits: the decode kernels that read it from global memory
DEC_CONFIGS = dict(CONFIGS, pq14_luv8=(1, 14, 0, 8, 1e4, 0.005))


@pytest.mark.parametrize("name", sorted(DEC_CONFIGS))
def test_decode_f16_equals_narrowed_float_decode(L, name):
    import torch
    cfg = DEC_CONFIGS[name]
    rng = np.random.default_rng(len(name))
    seen = dict(inf=0, nan=0, den=0)
    c = ctx(L, cfg)
    for profile in range(4):
        for (w, h) in DEC_SIZES:
            # sc 0.01 / 3e5 / 0 / NaN: results beyond 65504 (inf), in the binary16 denormal range, x / 0 and NaN
            for sc in (_sc_for(cfg), 0.01, 3e5, 0.0, float("nan")):
                nf = 3
                pl, st, pfs = _random_buffers(rng, w, h, profile, nf)
                tp = _tensor_u8(pl)
                ptrs = [t.data_ptr() for t in tp]
                n = w * h
                ref = torch.empty(nf * 3 * n, dtype=torch.float32, device=dev())
                c.decode_frames_device(ptrs, st, pfs, nf, w, h, profile, sc, ref.data_ptr(), 3 * n)
                # packed frames of halves with a frame stride of 3*n + 2 (two pixels per access; the gap must stay untouched)
                fs = 3 * n + 2
                o16 = torch.full((nf * fs,), 7, dtype=torch.int16, device=dev())
                c.decode_frames_device_f16(ptrs, st, pfs, nf, w, h, profile, sc, o16.data_ptr(), fs)
                # planar: three separate buffers
                pp = [torch.empty(nf * n, dtype=torch.float16, device=dev()) for _ in range(3)]
                c.decode_frames_device_planar_f16(ptrs, st, pfs, nf, w, h, profile, sc, [t.data_ptr() for t in pp], n)
                c.sync()
                r = ref.cpu().numpy()
                exp = float_to_half_np(r).reshape(nf, 3, n)
                got = o16.cpu().numpy().view(np.uint16).reshape(nf, fs)
                assert np.array_equal(got[:, :3 * n].reshape(nf, 3, n), exp), (name, profile, w, h, sc)
                assert np.all(got[:, 3 * n:] == 7), "wrote past the frame"
                for ch in range(3):
                    g = pp[ch].cpu().numpy().view(np.uint16).reshape(nf, n)
                    assert np.array_equal(g, exp[:, ch, :]), (name, profile, w, h, sc, "planar", ch)
                # host form, frame 0
                hpl = [pl[p][:pfs[p]].reshape(-1, st[p]) for p in range(3)]
                hg = c.decode_frame_f16(hpl, st, w, h, sc, profile)
                assert np.array_equal(hg.view(np.uint16).reshape(3, n), exp[0]), (name, profile, w, h, sc, "host")
                e = exp & 0x7fff
                seen["inf"] += int((e == 0x7c00).sum())
                seen["nan"] += int((e > 0x7c00).sum())
                seen["den"] += int(((e > 0) & (e < 0x400)).sum())
    assert seen["inf"] > 0 and seen["den"] > 0 and seen["nan"] > 0, seen


# ---- 3. encode from halves
def _half_frames(rng, nf, w, h):
    """nf (3,h,w) frames of halves: log-uniform positives, random bit patterns, and the special values"""
    f = np.exp(rng.uniform(np.log(1e-4), np.log(3e4), size=(nf, 3, h, w))).astype(np.float16)
    u = f.view(np.uint16)
    mask = rng.random(size=u.shape) < 0.15
    u[mask] = rng.integers(0, 1 << 16, size=int(mask.sum()), dtype=np.uint16)
    sp = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 65504.0, 2.0 ** -24, -2.0, -65504.0, 2.0 ** -14, 1.0],
                  dtype=np.float16)
    flat = f.reshape(nf, 3, -1)
    k = min(sp.size, flat.shape[2])
    for c in range(3):
        flat[:, c, :k] = np.roll(sp, c)[:k]
    return f


def _same_stats(a, b):
    """per-frame {sum, min, max}: min / max bit for bit; the sum is a float atomic sum, whose last bits (and NaN payload)
    depend on the arrival order of the workgroups' partial sums, for the float call as much as for the f16 one"""
    a, b = a.reshape(-1, 3), b.reshape(-1, 3)
    if not np.array_equal(a[:, 1:].view(np.uint32), b[:, 1:].view(np.uint32)):
        return False
    return bool(np.all((np.isnan(a[:, 0]) & np.isnan(b[:, 0])) | np.isclose(a[:, 0], b[:, 0], rtol=1e-5, atol=0)))


ENC_CASES = [  # (cfg, force_literal, expected search mode)
    ((1, 11, 0, 8, 1e4, 0.005), False, 3),      # PQ-11 Lu'v': records in LDS
    ((1, 11, 0, 8, 1e4, 0.005), True, 0),       # literal search, table in LDS
    ((1, 14, 0, 8, 1e4, 0.005), False, 4),      # PQ-14: records in global memory
    ((1, 14, 0, 8, 1e4, 0.005), True, 2),       # literal search, table in global memory
    ((1, 15, 1, 8, 1e4, 0.005), False, None),   # PQ-15 RGB
    ((1, 16, 3, 10, 1e4, 0.005), False, None),  # PQ-16 XYZ
    ((4, 12, 3, 8, 1e4, 0.005), False, 7),      # PTF_LINEAR: value-keyed records
    ((2, 12, 0, 8, 1e4, 0.005), False, None),   # LOG-12
    ((1, 10, 2, 10, 1000.0, 0.01), False, None),  # HDR10 Y'CbCr
]


def _encode_pair(c, frames16, w, h, profile, sc, stats, planar=False):
    """planes (+stats) of the float call on the widened frames and of the f16 call on the halves"""
    import torch
    nf = frames16.shape[0]
    n = w * h
    _, hs, st, _ = L_geometry(w, h, profile)
    sizes = [hs[p] * st[p] for p in range(3)]
    x16 = torch.from_numpy(frames16.reshape(-1).view(np.int16).copy()).to(dev())
    x32 = torch.from_numpy(_widen(frames16).reshape(-1)).to(dev())
    outs = []
    for half in (False, True):
        pl = [torch.zeros(nf * sizes[p], dtype=torch.uint8, device=dev()) for p in range(3)]
        sd = torch.zeros(3 * nf, dtype=torch.float32, device=dev()) if stats else None
        sp = sd.data_ptr() if stats else None
        pp = [t.data_ptr() for t in pl]
        if not half:
            c.encode_frames_device(x32.data_ptr(), 3 * n, nf, w, h, sc, profile, pp, st, sizes, sp)
        elif planar:
            base = x16.data_ptr()
            c.encode_frames_device_planar_f16([base, base + 2 * n, base + 4 * n], 3 * n, nf, w, h, sc, profile, pp, st, sizes, sp)
        else:
            c.encode_frames_device_f16(x16.data_ptr(), 3 * n, nf, w, h, sc, profile, pp, st, sizes, sp)
        c.sync()
        outs.append(([t.cpu().numpy() for t in pl], sd.cpu().numpy() if stats else None))
    return outs, st, sizes, hs


@pytest.mark.parametrize("case", range(len(ENC_CASES)))
def test_encode_f16_equals_float_encode_and_oracle(L, oracle_mod, case):
    cfg, literal, mode = ENC_CASES[case]
    o = oracle_mod
    c = ctx(L, cfg, literal=literal)
    if mode is not None:
        assert c.quantizer_info()["mode"] == mode
    orc = o.Oracle(*cfg)
    rng = np.random.default_rng(100 + case)
    scs = (1.0, 20.0) if cfg[2] == 2 else (1.0,)
    for profile in range(4):
        for w, h in ((258, 10), (256, 8), (34, 6), (6, 4)):   # (256: four pixels per thread; the others two)
            for sc in scs:
                for stats in (False, True):
                    fr = _half_frames(rng, 2, w, h)
                    (f32, f16), st, sizes, hs = _encode_pair(c, fr, w, h, profile, sc, stats, planar=(w == 34))
                    for p in range(3):
                        assert np.array_equal(f16[0][p], f32[0][p]), (cfg, literal, profile, w, sc, stats, p)
                    if stats:
                        assert _same_stats(f16[1], f32[1]), (cfg, profile, w, sc, f16[1], f32[1])
                    # the oracle, frame 1
                    ep, _, _ = orc.encode(_widen(fr[1]), sc, profile)
                    bps = 2 if profile > 1 else 1
                    sub = profile in (0, 2)
                    rb = (w * bps, (w // 2 if sub else w) * bps, (w // 2 if sub else w) * bps)
                    for p in range(3):
                        got = f16[0][p][sizes[p]:].reshape(hs[p], st[p])
                        assert np.array_equal(got[:, :rb[p]], ep[p][:, :rb[p]]), (cfg, literal, profile, w, sc, p, "oracle")
    # the host form on one frame (6 B per pixel up)
    fr = _half_frames(rng, 1, 258, 10)[0]
    a = c.encode_frame_f16(fr, scs[-1], 2)
    b = c.encode_frame(_widen(fr), scs[-1], 2)
    for p in range(3):
        assert np.array_equal(a[0][p], b[0][p])
    assert a[2] == pytest.approx(b[2], rel=1e-5, nan_ok=True)   # (mean luminance: an atomic sum, see _same_stats)


def test_ycbcr_f16_takes_the_half_table_by_type(L):
    """HDR10: frames of halves without statistics take the half-input table kernels at once (no probe, no backoff); with
    statistics the general kernels; a (sc, maxLum) without a table (sc = 0) the general kernels -- same planes throughout"""
    import torch
    from lumahdrv_amd import capi
    cfg = CONFIGS["pq10_ycbcr10"]
    rng = np.random.default_rng(5)
    assert capi.ycbcr_half_table(0.0, cfg[4]) is None
    for sc in (1.0, 20.0, 0.0):
        for stats in (False, True):
            fr = _half_frames(rng, 2, 258, 10)
            c = ctx(L, cfg)
            (f32, f16), st, sizes, _ = _encode_pair(c, fr, 258, 10, 2, sc, stats)
            for p in range(3):
                assert np.array_equal(f16[0][p], f32[0][p]), (sc, stats, p)
            if stats:
                assert _same_stats(f16[1], f32[1]), (sc, f16[1], f32[1])
            # the f16 call alone on a fresh context: the table kernel on its first launch exactly when it exists and no
            # statistics are asked for
            c = ctx(L, cfg)
            x16 = torch.from_numpy(fr.reshape(-1).view(np.int16).copy()).to(dev())
            pl = [torch.zeros(2 * sizes[p], dtype=torch.uint8, device=dev()) for p in range(3)]
            sd = torch.zeros(6, dtype=torch.float32, device=dev())
            c.encode_frames_device_f16(x16.data_ptr(), 3 * 258 * 10, 2, 258, 10, sc, 2, [t.data_ptr() for t in pl], st, sizes,
                                       sd.data_ptr() if stats else None)
            c.sync()
            for p in range(3):
                assert np.array_equal(pl[p].cpu().numpy(), f32[0][p]), (sc, stats, p, "alone")
            launches = c.half_table_info(20.0)["table_launches"]
            assert launches == (1 if sc > 0 and not stats else 0), (sc, stats, launches)


# ---- 4. full size
def test_full_size_4k(L):
    import torch
    w, h = 3840, 2160
    n = w * h
    for name, nf, sc in (("pq11_luv8", 8, 1.0), ("pq10_ycbcr10", 1, 20.0)):
        cfg = CONFIGS[name]
        c = ctx(L, cfg)
        g = torch.Generator(device=dev())
        g.manual_seed(3)
        x32 = torch.exp(torch.empty(nf * 3 * n, device=dev()).uniform_(np.log(1e-3), np.log(2e4), generator=g))
        x16 = x32.to(torch.float16)
        x32 = x16.to(torch.float32)
        _, hs, st, _ = L_geometry(w, h, 2)
        sizes = [hs[p] * st[p] for p in range(3)]
        res = []
        for half in (False, True):
            pl = [torch.zeros(nf * sizes[p], dtype=torch.uint8, device=dev()) for p in range(3)]
            pp = [t.data_ptr() for t in pl]
            if half:
                c.encode_frames_device_f16(x16.data_ptr(), 3 * n, nf, w, h, sc, 2, pp, st, sizes)
            else:
                c.encode_frames_device(x32.data_ptr(), 3 * n, nf, w, h, sc, 2, pp, st, sizes)
            c.sync()
            res.append(pl)
        for p in range(3):
            assert torch.equal(res[0][p], res[1][p]), (name, p)
        pp = [t.data_ptr() for t in res[0]]
        d32 = torch.empty(nf * 3 * n, dtype=torch.float32, device=dev())
        d16 = torch.empty(nf * 3 * n, dtype=torch.float16, device=dev())
        c.decode_frames_device(pp, st, sizes, nf, w, h, 2, sc, d32.data_ptr(), 3 * n)
        c.decode_frames_device_f16(pp, st, sizes, nf, w, h, 2, sc, d16.data_ptr(), 3 * n)
        c.sync()
        exp = float_to_half_torch(d32.view(torch.int32))
        assert torch.equal(d16.view(torch.int16), exp), name


# ---- 5. exhaustive narrowing on the device
def float_to_half_torch(bits32):
    """float_to_half_np on the GPU: int32 bit patterns -> int16 bit patterns (ExrInterface::floatToHalf)"""
    import torch
    b = bits32.to(torch.int64) & 0xffffffff
    sign = (b >> 16) & 0x8000
    e = (b >> 23) & 0xff
    m = b & 0x7fffff
    he = e - 112
    r = (he << 10) | (m >> 13)
    rem = m & 0x1fff
    r = r + ((rem > 0x1000) | ((rem == 0x1000) & ((r & 1) == 1))).to(torch.int64)
    den = (he <= 0) & (he >= -10)
    shift = torch.where(den, 14 - he, torch.ones_like(he))
    mm = m | 0x800000
    q = mm >> shift
    rr = mm & ((torch.ones_like(shift) << shift) - 1)
    hw = torch.ones_like(shift) << (shift - 1)
    rd = q + ((rr > hw) | ((rr == hw) & ((q & 1) == 1))).to(torch.int64)
    out = torch.zeros_like(b)
    out = torch.where((he > 0) & (he < 31), r, out)
    out = torch.where(den, rd, out)
    out = torch.where((he >= 31) & (e != 255), torch.full_like(b, 0x7c00), out)
    out = torch.where(e == 255, torch.where(m != 0, 0x7e00 | (m >> 13), torch.full_like(b, 0x7c00)), out)
    out = out | sign
    return torch.where(out >= 0x8000, out - 0x10000, out).to(torch.int16)


def test_device_narrowing_equals_float_to_half_for_every_float(L):
    import torch
    c = L.Context(0)
    s = torch.cuda.current_stream().cuda_stream
    c.set_stream(s)
    n = 1 << 26
    out = torch.empty(n, dtype=torch.int16, device=dev())
    base = torch.arange(n, dtype=torch.int64, device=dev())
    bad = 0
    for chunk in range(64):
        first = chunk * n
        c.f16_narrow_probe_device(out.data_ptr(), first, n)
        bits = (base + first)
        bits32 = torch.where(bits >= (1 << 31), bits - (1 << 32), bits).to(torch.int32)
        bad += int((out != float_to_half_torch(bits32)).sum().item())
    c.set_stream(None)
    assert bad == 0
    # and the torch port against the numpy restatement on a sample
    x = np.arange(0, 1 << 32, 65521, dtype=np.uint64).astype(np.uint32)
    t = float_to_half_torch(torch.from_numpy(x.view(np.int32)).to(dev())).cpu().numpy().view(np.uint16)
    assert np.array_equal(t, float_to_half_np(x.view(np.float32)))


# ---- 6. torch.float16 tensors as device buffers
def test_torch_float16_buffers_both_ways(L):
    import torch
    cfg = CONFIGS["pq11_luv8"]
    c = ctx(L, cfg)
    w, h, nf = 256, 64, 2
    x = (torch.rand(nf, 3, h, w, device=dev()) * 1000 + 0.01).to(torch.float16)
    _, hs, st, _ = L_geometry(w, h, 2)
    sizes = [hs[p] * st[p] for p in range(3)]
    a = [torch.zeros(nf * sizes[p], dtype=torch.uint8, device=dev()) for p in range(3)]
    b = [torch.zeros(nf * sizes[p], dtype=torch.uint8, device=dev()) for p in range(3)]
    c.encode_frames_device_f16(x.data_ptr(), 3 * w * h, nf, w, h, 1.0, 2, [t.data_ptr() for t in a], st, sizes)
    xf = x.float().contiguous()
    c.encode_frames_device(xf.data_ptr(), 3 * w * h, nf, w, h, 1.0, 2, [t.data_ptr() for t in b], st, sizes)
    y16 = torch.empty(nf, 3, h, w, dtype=torch.float16, device=dev())
    y32 = torch.empty(nf, 3, h, w, dtype=torch.float32, device=dev())
    c.decode_frames_device_f16([t.data_ptr() for t in a], st, sizes, nf, w, h, 2, 1.0, y16.data_ptr(), 3 * w * h)
    c.decode_frames_device([t.data_ptr() for t in a], st, sizes, nf, w, h, 2, 1.0, y32.data_ptr(), 3 * w * h)
    c.sync()
    for p in range(3):
        assert torch.equal(a[p], b[p])
    assert torch.equal(y16.view(torch.int16).flatten(), float_to_half_torch(y32.view(torch.int32).flatten()))
    # LumaFrameCodec's host forms
    codec = L.LumaFrameCodec(ctx=c)
    f16 = x[0].cpu().numpy()
    planes, strides, mean = codec.encode_half(f16)
    planes2, _, mean2 = codec.encode(f16.astype(np.float32))
    for p in range(3):
        assert np.array_equal(planes[p], planes2[p])
    assert mean == pytest.approx(mean2, rel=1e-5)
    dh = codec.decode_half(planes, strides, w, h)
    assert dh.dtype == np.float16
    assert np.array_equal(dh.view(np.uint16), float_to_half_np(codec.decode(planes, strides, w, h)))


# ---- 7. argument errors
def test_f16_argument_errors(L):
    import torch
    from lumahdrv_amd import capi
    c = ctx(L, CONFIGS["pq11_luv8"])
    w, h = 64, 16
    _, hs, st, _ = L_geometry(w, h, 2)
    sizes = [hs[p] * st[p] for p in range(3)]
    pl = [torch.zeros(sizes[p], dtype=torch.uint8, device=dev()) for p in range(3)]
    pp = [t.data_ptr() for t in pl]
    buf = torch.zeros(3 * w * h + 8, dtype=torch.float16, device=dev())
    base = buf.data_ptr()
    for call in (lambda: c.encode_frames_device_f16(base + 2, 3 * w * h, 1, w, h, 1.0, 2, pp, st, sizes),
                 lambda: c.decode_frames_device_f16(pp, st, sizes, 1, w, h, 2, 1.0, base + 2, 3 * w * h),
                 lambda: c.encode_frames_device_f16(base, 3 * w * h + 1, 2, w, h, 1.0, 2, pp, st, sizes),
                 lambda: c.decode_frames_device_planar_f16(pp, st, sizes, 1, w, h, 2, 1.0, [base, base + 2 * w * h + 2, base + 4 * w * h], w * h),
                 lambda: c.encode_frames_device_planar_f16([base + 6, base + 2 * w * h, base + 4 * w * h], w * h, 1, w, h, 1.0, 2, pp, st, sizes),
                 lambda: c.f16_narrow_probe_device(base, 0, 3)):
        with pytest.raises(capi.LumaHipError) as e:
            call()
        assert e.value.code == capi.ERR_ARG
    c.sync()
    fresh = L.Context(0)
    for call in (lambda: fresh.encode_frames_device_f16(base, 3 * w * h, 1, w, h, 1.0, 2, pp, st, sizes),
                 lambda: fresh.decode_frames_device_f16(pp, st, sizes, 1, w, h, 2, 1.0, base, 3 * w * h),
                 lambda: fresh.encode_frame_f16(np.zeros((3, h, w), dtype=np.float16)),
                 lambda: fresh.decode_frame_f16([np.zeros(s, np.uint8) for s in sizes], st, w, h)):
        with pytest.raises(capi.LumaHipError) as e:
            call()
        assert e.value.code == capi.ERR_STATE
