"""Code-domain distortion (include/lumahip.h lumahip_distortion_frames_device / _planar / _f16 / _planar_f16 /
lumahip_distortion_frame_host): per frame and plane {sse, sad, max_abs, n_differ} of the planes the encode call would write
against GIVEN planes.  Every expectation is exact equality of all twelve integers per frame.

1. The reference's planes (tests/golden/ref_planes.npz): `_in` against `_plane*` is all zeros, against the garbled `_dec_plane*`
   it is numpy's sums over the two sets.
2. Against lumahip_encode_frames_device: its planes, perturbed on the host, six configurations x profiles 0-3 x sizes (34,18)
   (258,6) (64,32) (6,4) x 3 frames x preScalings {1, 20, 0.01}; sentinel bytes in every gap; the planar and binary16 forms.
3. Accumulator width (one wave carries more than 2^32).  4. Persistent loop and frame change (2 workgroups of 64 threads).
5. Unordered section, one 1280x720 frame, repeatability, inputs untouched.  6. The host form.  7. Errors: nothing is launched.
"""
import os

import numpy as np
import pytest

from tests.golden.make_golden import CONFIGS
from tests.test_distortion_host import expected_distortion, fixture_keys, key_parts

pytestmark = pytest.mark.gpu

CFG = dict(CONFIGS, linear12_luv8=(4, 12, 0, 8, 1e4, 0.005), pq14_luv8=(1, 14, 0, 8, 1e4, 0.005))
SENTINEL = 0xC3
GAP = 48          # bytes between one frame's plane and the next frame's
OUT_FILL = -0x3C3C3C3C3C3C3C3D   # what out_dev holds before a call (int64 view of 0xC3C3...C3)
SIZES = [(34, 18), (258, 6), (64, 32), (6, 4)]
ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = 1, 3, 4


@pytest.fixture(scope="module")
def L():
    import lumahdrv_amd
    return lumahdrv_amd


def _dev():
    import torch
    return torch.device("cuda:0")


def _ctx(L, cfg, literal=False, quantizer=True):
    """a context on torch's current stream, so that its launches are ordered with the tensors' fills and copies"""
    import torch
    c = L.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    if literal:
        c.tune("force_literal", 1)
    if quantizer:
        c.set_quantizer(*cfg, L.build_lut(cfg[0], cfg[1], cfg[4], cfg[5]))
    return c


def _frames(rng, nf, w, h, halves=False):
    """nf (3,h,w) float32 frames: log-uniform positives with zeros, negatives and large values mixed in"""
    f = np.exp(rng.uniform(np.log(1e-4), np.log(3e4), size=(nf, 3, h, w))).astype(np.float32)
    m = rng.random(size=f.shape)
    f[m < 0.02] = 0.0
    f[(m >= 0.02) & (m < 0.04)] *= -1.0
    f[(m >= 0.04) & (m < 0.05)] = 6.5e4
    return f.astype(np.float16).astype(np.float32) if halves else f


class Frames:
    """frames on the device, frame f at base + f * fs elements; the gap between frames holds sentinel bytes"""

    def __init__(self, frames, dtype=np.float32, pad=4):
        import torch
        nf, _, h, w = frames.shape
        self.nf, self.w, self.h, self.n = nf, w, h, w * h
        self.fs = 3 * self.n + pad
        buf = np.full(nf * self.fs * np.dtype(dtype).itemsize, SENTINEL, dtype=np.uint8).view(dtype).reshape(nf, self.fs)
        buf[:, :3 * self.n] = frames.reshape(nf, -1).astype(dtype)
        self.host = buf.copy()
        self.t = torch.from_numpy(buf.view(np.uint8).ravel().copy()).to(_dev())

    @property
    def ptr(self):
        return self.t.data_ptr()

    def unchanged(self):
        return np.array_equal(self.t.cpu().numpy(), self.host.view(np.uint8).ravel())


class Planes:
    """nf frames of code planes on the device: plane p of frame f at buf[p] + f * pfs[p], rows st[p] bytes apart"""

    def __init__(self, L, w, h, profile, nf, fill=None, strides=None, gap=GAP):
        import torch
        self.w, self.h, self.profile, self.nf = w, h, profile, nf
        _, hs, st, _ = L.plane_geometry(w, h, profile)
        self.st = tuple(int(s) for s in strides) if strides is not None else st
        self.hs = hs
        self.size = [hs[p] * self.st[p] for p in range(3)]
        self.pfs = [self.size[p] + gap for p in range(3)]
        if fill is None:
            fill = [np.full(nf * self.pfs[p], SENTINEL, dtype=np.uint8) for p in range(3)]
        self.fill = [np.ascontiguousarray(f) for f in fill]
        self.t = [torch.from_numpy(self.fill[p]).to(_dev()) for p in range(3)]

    @property
    def ptrs(self):
        return [t.data_ptr() for t in self.t]

    def host(self):
        return [t.cpu().numpy() for t in self.t]

    def frame(self, bufs, f):
        """frame f as three (rows, stride) arrays"""
        return [bufs[p][f * self.pfs[p]: f * self.pfs[p] + self.size[p]].reshape(self.hs[p], self.st[p]) for p in range(3)]

    def unchanged(self):
        return all(np.array_equal(a, b) for a, b in zip(self.host(), self.fill))


def _from_frames(L, frames, w, h, profile, strides=None):
    """Planes holding the given frames (lists of three (rows, >= row bytes) arrays), sentinel bytes in every gap"""
    pl = Planes(L, w, h, profile, len(frames), strides=strides)
    fill = [np.full(len(frames) * pl.pfs[p], SENTINEL, dtype=np.uint8) for p in range(3)]
    for f, fr in enumerate(frames):
        for p in range(3):
            rb = _row_bytes(w, h, profile, p)
            dst = fill[p][f * pl.pfs[p]: f * pl.pfs[p] + pl.size[p]].reshape(pl.hs[p], pl.st[p])
            dst[:, :rb] = np.asarray(fr[p])[:pl.hs[p], :rb]
    return Planes(L, w, h, profile, len(frames), fill=fill, strides=strides)


def _row_bytes(w, h, profile, p):
    sub, bps = profile in (0, 2), 2 if profile > 1 else 1
    return (w // 2 if (p and sub) else w) * bps


def _perturb(rng, planes, w, h, profile, frac=0.10, amp=7, extremes=3):
    """a copy of one frame's planes with +-1 .. +-amp on about `frac` of the samples and a few 0 / 0xFFFF (0xFF) samples"""
    out = []
    bps = 2 if profile > 1 else 1
    top = 0xFFFF if bps == 2 else 0xFF
    for p in range(3):
        a = np.array(planes[p], copy=True)
        rows, rb = a.shape[0], _row_bytes(w, h, profile, p)
        s = np.ascontiguousarray(a[:, :rb]).view("<u2" if bps == 2 else np.uint8).astype(np.int64)
        hit = rng.random(size=s.shape) < frac
        delta = rng.integers(1, amp + 1, size=s.shape) * rng.choice([-1, 1], size=s.shape)
        s = np.clip(s + hit * delta, 0, top)
        for _ in range(extremes):
            s[rng.integers(0, rows), rng.integers(0, s.shape[1])] = rng.choice([0, top])
        a[:, :rb] = s.astype("<u2" if bps == 2 else np.uint8).view(np.uint8).reshape(rows, rb)
        out.append(a)
    return out


def _out(nf):
    import torch
    return torch.full((nf * 12,), OUT_FILL, dtype=torch.int64, device=_dev())


def _words(out, nf):
    return out.cpu().numpy().view(np.uint64).reshape(nf, 3, 4)


def _dist(c, fr, sc, given, form="packed"):
    """the twelve words per frame of the device call in one of its four forms"""
    import torch
    out = _out(fr.nf)
    args = (fr.fs, fr.nf, fr.w, fr.h, sc, given.profile, given.ptrs, given.st, given.pfs, out.data_ptr())
    esz = fr.t.element_size() * fr.host.dtype.itemsize
    planar = [fr.ptr + k * fr.n * esz for k in range(3)]
    if form == "packed":
        c.distortion_frames_device(fr.ptr, *args)
    elif form == "planar":
        c.distortion_frames_device_planar(planar, *args)
    elif form == "f16":
        c.distortion_frames_device_f16(fr.ptr, *args)
    else:
        c.distortion_frames_device_planar_f16(planar, *args)
    torch.cuda.synchronize()
    return _words(out, fr.nf)


def _encode(c, L, fr, sc, profile, strides=None):
    """the planes lumahip_encode_frames_device writes for these frames, as host buffers + their Planes"""
    import torch
    pl = Planes(L, fr.w, fr.h, profile, fr.nf, strides=strides)
    c.encode_frames_device(fr.ptr, fr.fs, fr.nf, fr.w, fr.h, sc, profile, pl.ptrs, pl.st, pl.pfs)
    torch.cuda.synchronize()
    return pl, pl.host()


def _expect(enc, ebufs, given, w, h, profile):
    return np.stack([expected_distortion(enc.frame(ebufs, f), given.frame(given.fill, f), w, h, profile) for f in range(enc.nf)])


# ---- 1. the reference's planes
def test_reference_planes_and_their_garbled_copies(L, golden_dir):
    gp = np.load(os.path.join(golden_dir, "ref_planes.npz"))
    keys = fixture_keys(gp)
    assert len(keys) == 16
    for key in keys:
        name, w, h, profile = key_parts(key)
        cfg = CONFIGS[name]
        sc = 20.0 if cfg[2] == 2 else 1.0
        c = _ctx(L, cfg)
        fr = Frames(gp[key + "_in"][None])
        pl = [gp[key + "_plane%d" % p] for p in range(3)]
        dpl = [gp[key + "_dec_plane%d" % p] for p in range(3)]
        same = _from_frames(L, [pl], w, h, profile, strides=gp[key + "_stride"])
        got = _dist(c, fr, sc, same)
        assert not got.any(), (key, got)
        garbled = _from_frames(L, [dpl], w, h, profile, strides=gp[key + "_dec_stride"])
        got = _dist(c, fr, sc, garbled)
        exp = expected_distortion(pl, dpl, w, h, profile)
        assert exp.any() and np.array_equal(got[0], exp), (key, got, exp)
        assert np.array_equal(c.distortion_frame(gp[key + "_in"], dpl, garbled.st, sc, profile), exp), (key, "host")


# ---- 2. against the existing encode call
ENC_CASES = ["pq11_luv8", "log12_luv8", "linear12_luv8", "pq10_ycbcr10", "pq12_rgb", "linear12_xyz"]


@pytest.mark.parametrize("name", ENC_CASES)
def test_equals_numpy_on_the_encode_calls_planes(L, name):
    cfg = CFG[name]
    rng = np.random.default_rng(len(name) * 7 + cfg[1])
    c = _ctx(L, cfg)
    nf = 3
    scs = (1.0, 20.0, 0.01)
    first = True
    for profile in range(4):
        for i, (w, h) in enumerate(SIZES):
            sc = scs[(i + profile) % 3]
            fr = Frames(_frames(rng, nf, w, h), pad=4 if i % 2 == 0 else 2)
            enc, ebufs = _encode(c, L, fr, sc, profile)
            if first:
                first = False
                mode = c.quantizer_info()["mode"]
                if mode not in (3, 7):   # ("where its records are in LDS": anything else is refused)
                    with pytest.raises(L.LumaHipError) as ei:
                        _dist(c, fr, sc, enc)
                    assert ei.value.code == ERR_UNSUPPORTED
                    return
                if name == "linear12_luv8":
                    assert mode == 7
            given = _from_frames(L, [_perturb(rng, enc.frame(ebufs, f), w, h, profile) for f in range(nf)], w, h, profile)
            exp = _expect(enc, ebufs, given, w, h, profile)
            assert exp[:, :, 3].any(axis=1).all(), "every frame differs somewhere"
            got = _dist(c, fr, sc, given)
            assert np.array_equal(got, exp), (name, profile, w, h, sc, got, exp)
            assert not _dist(c, fr, sc, enc).any(), (name, profile, w, h, sc, "its own planes")
            assert fr.unchanged() and given.unchanged()
            # rows the vector loads cannot take: odd strides
            if profile in (1, 2) and (w, h) != (6, 4):
                odd = _from_frames(L, [given.frame(given.fill, f) for f in range(nf)], w, h, profile,
                                   strides=[given.st[p] + 3 for p in range(3)])
                assert np.array_equal(_dist(c, fr, sc, odd), exp), (name, profile, w, h, "odd strides")


@pytest.mark.parametrize("name,half_table", [("pq11_luv8", 1), ("pq12_rgb", 1), ("pq10_ycbcr10", 2), ("pq10_ycbcr10", 0)])
def test_planar_and_binary16_forms_equal_the_float_call(L, name, half_table):
    cfg = CFG[name]
    rng = np.random.default_rng(11 + half_table)
    c = _ctx(L, cfg)
    c.tune("half_table", half_table)
    nf = 3
    for profile in (2, 3, 0):
        for (w, h) in SIZES:
            sc = 20.0 if cfg[2] == 2 else 1.0
            frames = _frames(rng, nf, w, h, halves=True)
            fr = Frames(frames)
            fr16 = Frames(frames, dtype=np.float16)
            enc, ebufs = _encode(c, L, fr, sc, profile)
            given = _from_frames(L, [_perturb(rng, enc.frame(ebufs, f), w, h, profile) for f in range(nf)], w, h, profile)
            exp = _expect(enc, ebufs, given, w, h, profile)
            for form, src in (("packed", fr), ("planar", fr), ("f16", fr16), ("planar_f16", fr16)):
                got = _dist(c, src, sc, given, form)
                assert np.array_equal(got, exp), (name, half_table, profile, w, h, form, got, exp)
            assert fr16.unchanged()
    if cfg[2] == 2:
        info = c.half_table_info(20.0)
        assert info["used"] == (half_table != 0)


# ---- 3. accumulator width: one wave carries more than 2^32 of squared difference per plane
def test_one_wave_accumulates_beyond_32_bits(L):
    c = _ctx(L, CFG["pq11_luv8"])
    c.tune("grid_enc", 1)
    c.tune("block", 64)
    rng = np.random.default_rng(3)
    w, h, nf, profile = 64, 32, 3, 2
    fr = Frames(_frames(rng, nf, w, h))
    enc, ebufs = _encode(c, L, fr, 1.0, profile)
    ones = Planes(L, w, h, profile, nf, fill=[np.full(nf * enc.pfs[p], 0xFF, dtype=np.uint8) for p in range(3)])
    exp = _expect(enc, ebufs, ones, w, h, profile)
    assert np.all(exp[:, :, 0] > np.uint64(1) << np.uint64(32))
    got = _dist(c, fr, 1.0, ones)
    assert np.array_equal(got, exp), (got, exp)


# ---- 4. persistent loop and frame change
@pytest.mark.parametrize("size", [(6, 4), (258, 6)])
def test_two_workgroups_book_every_frame_to_itself(L, size):
    w, h = size
    rng = np.random.default_rng(w)
    nf = 3
    for name, profile in (("pq11_luv8", 2), ("pq10_ycbcr10", 3), ("pq12_rgb", 0)):
        cfg = CFG[name]
        sc = 20.0 if cfg[2] == 2 else 1.0
        c = _ctx(L, cfg)
        c.tune("grid_enc", 2)
        c.tune("block", 64)
        fr = Frames(_frames(rng, nf, w, h))
        enc, ebufs = _encode(c, L, fr, sc, profile)
        # frame f: its own share of perturbed samples and its own amplitude
        given = _from_frames(L, [_perturb(rng, enc.frame(ebufs, f), w, h, profile, frac=0.2 + 0.3 * f, amp=1 + 3 * f, extremes=f)
                                 for f in range(nf)], w, h, profile)
        exp = _expect(enc, ebufs, given, w, h, profile)
        assert len({tuple(e.ravel()) for e in exp}) == nf
        got = _dist(c, fr, sc, given)
        assert np.array_equal(got, exp), (name, size, got, exp)


# ---- 5. run-time behaviour
def test_unordered_section_two_batches_on_two_lanes(L):
    import torch
    c = _ctx(L, CFG["pq11_luv8"])
    rng = np.random.default_rng(5)
    w, h, nf, profile = 258, 6, 3, 2
    batches = []
    for _ in range(2):
        fr = Frames(_frames(rng, nf, w, h))
        enc, ebufs = _encode(c, L, fr, 1.0, profile)
        given = _from_frames(L, [_perturb(rng, enc.frame(ebufs, f), w, h, profile) for f in range(nf)], w, h, profile)
        batches.append((fr, given, _expect(enc, ebufs, given, w, h, profile), _out(nf)))
    torch.cuda.synchronize()
    c.begin_unordered(2)
    for fr, given, _, out in batches:
        c.distortion_frames_device(fr.ptr, fr.fs, nf, w, h, 1.0, profile, given.ptrs, given.st, given.pfs, out.data_ptr())
    c.end_unordered()
    c.sync()
    torch.cuda.synchronize()
    for fr, given, exp, out in batches:
        assert np.array_equal(_words(out, nf), exp)


@pytest.mark.parametrize("name", ["pq11_luv8", "pq10_ycbcr10"])
def test_one_720p_frame_twice(L, name):
    cfg = CFG[name]
    sc = 20.0 if cfg[2] == 2 else 1.0
    c = _ctx(L, cfg)
    rng = np.random.default_rng(720)
    w, h, profile = 1280, 720, 2
    fr = Frames(_frames(rng, 1, w, h))
    enc, ebufs = _encode(c, L, fr, sc, profile)
    given = _from_frames(L, [_perturb(rng, enc.frame(ebufs, 0), w, h, profile)], w, h, profile)
    exp = _expect(enc, ebufs, given, w, h, profile)
    a = _dist(c, fr, sc, given)
    b = _dist(c, fr, sc, given)
    assert np.array_equal(a, exp), (a, exp)
    assert np.array_equal(a, b)
    assert fr.unchanged() and given.unchanged()


# ---- 6. the host form
def test_host_form_equals_the_device_call(L):
    rng = np.random.default_rng(6)
    for name, profile, (w, h) in (("pq11_luv8", 2, (258, 6)), ("pq10_ycbcr10", 3, (34, 18)), ("linear12_luv8", 1, (64, 32))):
        cfg = CFG[name]
        sc = 20.0 if cfg[2] == 2 else 1.0
        c = _ctx(L, cfg)
        frames = _frames(rng, 1, w, h)
        fr = Frames(frames)
        enc, ebufs = _encode(c, L, fr, sc, profile)
        g = _perturb(rng, enc.frame(ebufs, 0), w, h, profile)
        given = _from_frames(L, [g], w, h, profile)
        dev = _dist(c, fr, sc, given)
        host = c.distortion_frame(frames[0], given.frame(given.fill, 0), given.st, sc, profile)
        assert host.dtype == np.uint64 and np.array_equal(host, dev[0]), (name, host, dev)
        assert dev.any()


# ---- 7. errors: nothing is launched, out_dev is left as it was
def test_errors_launch_nothing(L):
    import torch
    rng = np.random.default_rng(7)
    w, h, nf, profile = 34, 18, 1, 2
    frames = _frames(rng, nf, w, h)
    fr = Frames(frames)
    given = Planes(L, w, h, profile, nf)

    def refused(c, code, fr=fr, w=w, out_ptr="own", given=given):
        out = _out(nf)
        ptr = out.data_ptr() if out_ptr == "own" else out_ptr(out)
        with pytest.raises(L.LumaHipError) as ei:
            c.distortion_frames_device(fr.ptr, fr.fs, nf, w, h, 1.0, profile, given.ptrs, given.st, given.pfs, ptr)
        assert ei.value.code == code, ei.value
        torch.cuda.synchronize()
        assert np.all(out.cpu().numpy() == OUT_FILL)

    good = _ctx(L, CFG["pq11_luv8"])
    refused(_ctx(L, CFG["pq11_luv8"], quantizer=False), ERR_STATE)                  # no quantizer
    refused(good, ERR_ARG, w=33)                                                    # odd size
    refused(good, ERR_ARG, out_ptr=lambda o: o.data_ptr() + 4)                      # misaligned out_dev
    refused(good, ERR_ARG, out_ptr=lambda o: None)                                  # null out_dev
    refused(good, ERR_ARG, out_ptr=lambda o: given.ptrs[0] + 64)                    # out_dev inside a given plane
    refused(good, ERR_ARG, out_ptr=lambda o: fr.ptr + 8 * (w * h // 2))             # out_dev inside the frame
    refused(_ctx(L, CFG["pq11_luv8"], literal=True), ERR_UNSUPPORTED)               # force_literal
    refused(_ctx(L, CFG["pq14_luv8"]), ERR_UNSUPPORTED)                             # a 14-bit table: records in global memory
    assert fr.unchanged() and given.unchanged()
    # ... and the same arguments are accepted by a context that can
    assert _dist(good, fr, 1.0, given).shape == (1, 3, 4)
