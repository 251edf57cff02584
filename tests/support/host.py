"""What the tests share that needs numpy alone: no torch, no library.  Plane geometry, the numpy models the measuring calls are held to,
the readers of the fixtures in tests/golden, and the builders of the host byte buffers that tests/support/device.py puts on the GPU.

Helpers here assert with an explicit message: pytest rewrites `assert` in test modules only."""
import numpy as np

from tests.golden import make_transcode_golden as mg
from tests.golden.make_golden import CONFIGS

SENTINEL = 0xC3
GAP = 48          # bytes between one frame's plane and the next frame's
GUARD = 16        # words behind a map buffer, which a call must leave alone
OUT_FILL = -0x3C3C3C3C3C3C3C3D   # what out_dev / map_dev hold before a call (int64 view of 0xC3C3...C3)
BLOCKS = (16, 32, 64)
ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = 1, 3, 4

# the configurations, pairs and sizes the code-plane families share
CFG = dict(CONFIGS, linear12_luv8=(4, 12, 0, 8, 1e4, 0.005), pq14_luv8=(1, 14, 0, 8, 1e4, 0.005),
           pq10_ycbcr10_4000=mg.CONFIGS["pq10_ycbcr10_4000"])
ENC_CASES = ["pq11_luv8", "log12_luv8", "linear12_luv8", "pq10_ycbcr10", "pq12_rgb", "linear12_xyz"]
PAIRS = [("pq11_luv8", "pq10_ycbcr10"), ("pq11_luv8", "log12_luv8"), ("psi11_luv8", "linear12_luv8"), ("hdrvdp12_luv10", "pq11_luv8"),
         ("pq10_ycbcr10", "pq11_luv8"), ("pq10_ycbcr10", "pq10_ycbcr10_4000"), ("pq10_ycbcr10", "linear12_luv8"),
         ("log12_luv8", "psi11_luv8"), ("hdrvdp12_luv10", "pq10_ycbcr10")]
SIZES = [(34, 18), (258, 6), (64, 32), (6, 4)]
MAP_SIZES = [(34, 18), (260, 6), (258, 6), (264, 70), (64, 32), (6, 4)]


# ---- float helpers
def same_bits(a, b):
    a = np.asarray(a, dtype=np.float32)
    b = np.asarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def widen_halves(frames16):
    """binary16 -> float32 as IEEE conversion (and the kernels' v_cvt_f32_f16) widens: a signalling NaN comes out quiet.
    numpy's astype keeps it signalling, and a signalling NaN in the float kernels' min / max (v_min_f32 / v_max_f32 return
    NaN for one) would drop the values the wave had seen before it -- the float call would then be fed other data than the
    kernels of the f16 call read"""
    w = np.asarray(frames16).astype(np.float32)
    b = w.view(np.uint32)
    b[np.isnan(w)] |= np.uint32(0x00400000)
    return w


def float_to_half_np(x) -> np.ndarray:
    """ExrInterface::floatToHalf (lumahdrv_amd/csrc/facade/exr_interface.cpp) over a float32 array -> uint16 bit patterns"""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.int64)
    sign = (b >> 16) & 0x8000
    e = (b >> 23) & 0xff
    m = b & 0x7fffff
    he = e - 127 + 15
    out = np.zeros(b.shape, dtype=np.int64)
    # normal results (may round up into the next binade, or to infinity)
    r = (he << 10) | (m >> 13)
    rem = m & 0x1fff
    r = r + ((rem > 0x1000) | ((rem == 0x1000) & ((r & 1) == 1)))
    normal = (he > 0) & (he < 31)
    out[normal] = r[normal]
    # denormal results: shift the full significand with round-to-nearest-even
    den = (he <= 0) & (he >= -10)
    shift = np.where(den, 14 - he, 1)
    mm = m | 0x800000
    q = mm >> shift
    rr = mm & ((np.int64(1) << shift) - 1)
    hw = np.int64(1) << (shift - 1)
    rd = q + ((rr > hw) | ((rr == hw) & ((q & 1) == 1)))
    out[den] = rd[den]
    out[(he >= 31) & (e != 255)] = 0x7c00
    special = e == 255
    out[special] = np.where(m[special] != 0, 0x7e00 | (m[special] >> 13), 0x7c00)
    return (out | sign).astype(np.uint16)


def _half_policy_model(kinds, lag=4, longest=1024):
    """lumahip_core.hip lag_policy_next (LagPolicy, lumahip_internal.hpp) restated: kinds[i] = True when eligible launch i holds full-precision floats (a table launch on
    it reports).  Returns, per launch, (table launches so far, back-off launches so far) AFTER it was issued."""
    ON, BACKOFF, PROBE_WAIT = 0, 1, 2
    state, left, length, pending, table, backoff, out = ON, 0, 0, [], 0, 0, []
    for e, is_float in enumerate(kinds):
        while pending and pending[0][0] + lag <= e:
            _, reported, probe = pending.pop(0)
            if state == ON and reported:
                state, length = BACKOFF, 16
                left = length
            elif state == PROBE_WAIT and probe:
                if reported:
                    length = min(2 * max(length, 8), longest)
                    state, left = BACKOFF, length
                else:
                    state, length = ON, 0
        probe = False
        if state == BACKOFF and left > 0:
            left -= 1
            backoff += 1
        elif state == PROBE_WAIT:
            backoff += 1
        else:
            if state == BACKOFF:
                state, probe = PROBE_WAIT, True
            pending.append((e, is_float, probe))
            table += 1
        out.append((table, backoff))
    return out


# ---- plane geometry (independent arithmetic: nothing here asks the library)
def plane_rows(w, h, profile, p):
    """(rows, row bytes) of plane p: profiles 0 and 2 subsample the chroma planes, profiles 2 and 3 hold two bytes per sample"""
    sub, bps = profile in (0, 2), 2 if profile > 1 else 1
    return ((h + 1) // 2 if (p and sub) else h), ((w + 1) // 2 if (p and sub) else w) * bps


def per_plane(v):
    """a value per plane from one value or from three"""
    return tuple(v) if isinstance(v, (tuple, list)) else (v,) * 3


def layout(w, h, profile, st, gap=GAP):
    """(rows, bytes, frame stride) per plane, for rows st[p] bytes apart and `gap` bytes (one number, or one per plane) behind every
    frame's plane"""
    hs = [plane_rows(w, h, profile, p)[0] for p in range(3)]
    size = [hs[p] * st[p] for p in range(3)]
    return hs, size, [size[p] + per_plane(gap)[p] for p in range(3)]


def same_rows(a, b, w, h, profile):
    """two sets of three planes hold the same samples (their row paddings may differ)"""
    return all(np.array_equal(a[p][:, :plane_rows(w, h, profile, p)[1]], b[p][:, :plane_rows(w, h, profile, p)[1]]) for p in range(3))


# ---- the numpy models of the measuring calls
def plane_samples(plane, w, h, profile, p):
    """the samples of plane p -- a (rows, stride) uint8 array -- as a (rows, columns) integer array: one byte, or two bytes
    little-endian, over the sample columns only"""
    sub, bps = profile in (0, 2), 2 if profile > 1 else 1
    rows, cols = (h // 2, w // 2) if (p and sub) else (h, w)
    a = np.ascontiguousarray(np.asarray(plane)[:rows, :cols * bps])
    return (a.view("<u2") if bps == 2 else a).astype(np.int64)


def expected_distortion(planes_e, planes_g, w, h, profile):
    """(3, 4) uint64: per plane {sum (e-g)^2, sum |e-g|, max |e-g|, #(e != g)} of two sets of three (rows, stride) uint8 planes"""
    out = np.zeros((3, 4), dtype=np.uint64)
    for p in range(3):
        d = np.abs(plane_samples(planes_e[p], w, h, profile, p) - plane_samples(planes_g[p], w, h, profile, p)).astype(np.uint64)
        out[p] = (np.sum(d * d, dtype=np.uint64), np.sum(d, dtype=np.uint64), d.max(), np.count_nonzero(d))
    return out


def expected_distortion_map(planes_e, planes_g, w, h, profile, block):
    """(nby, nbx, 3, 4) uint64: expected_distortion per block of block x block luma pixels -- on a 4:2:0 chroma plane the
    block/2 x block/2 samples co-sited with them -- cut at the frame's edges"""
    nbx, nby = -(-w // block), -(-h // block)
    out = np.zeros((nby, nbx, 3, 4), dtype=np.uint64)
    for p in range(3):
        b = block // 2 if (p and profile in (0, 2)) else block
        d = np.abs(plane_samples(planes_e[p], w, h, profile, p) - plane_samples(planes_g[p], w, h, profile, p)).astype(np.uint64)
        for by in range(nby):
            for bx in range(nbx):
                t = d[by * b:(by + 1) * b, bx * b:(bx + 1) * b]
                assert t.size > 0, (p, by, bx, "a block without samples")
                out[by, bx, p] = (np.sum(t * t, dtype=np.uint64), np.sum(t, dtype=np.uint64), t.max(), np.count_nonzero(t))
    return out


def fold_map(m):
    """the (3, 4) words of a frame from its (nby, nbx, 3, 4) map: sum, sum, max, sum over the blocks"""
    out = m.sum(axis=(0, 1), dtype=np.uint64)
    out[:, 2] = m[:, :, :, 2].max(axis=(0, 1))
    return out


def expect(enc, ebufs, given, gbufs):
    """expected_distortion of every frame of two plane sets (anything with .frame(bufs, f), .nf, .w, .h, .profile) from their host buffers"""
    return np.stack([expected_distortion(enc.frame(ebufs, f), given.frame(gbufs, f), enc.w, enc.h, enc.profile) for f in range(enc.nf)])


def expect_map(enc, ebufs, given, gbufs, block):
    return np.stack([expected_distortion_map(enc.frame(ebufs, f), given.frame(gbufs, f), enc.w, enc.h, enc.profile, block)
                     for f in range(enc.nf)])


def nwords(nf, w, h, block):
    return nf * (-(-w // block)) * (-(-h // block)) * 12


def map_words(buf, nf, w, h, block):
    """the map of a call as (nf, nby, nbx, 3, 4) uint64, after checking the guard words behind it; buf: the nwords + GUARD int64 of
    tests/support/device.py map_buf, or a numpy array of them"""
    a = buf.cpu().numpy() if hasattr(buf, "cpu") else np.asarray(buf)
    assert np.all(a[-GUARD:] == OUT_FILL), "guard words behind the map"
    return a[:-GUARD].view(np.uint64).reshape(nf, -(-h // block), -(-w // block), 3, 4)


def neither_path_is_vacuous(exp, tag):
    """asserted on the numpy expectation: with more than one block column and row, every plane has a block without a difference and at
    least half of its blocks differ"""
    nd = exp[:, :, :, :, 3]                       # (nf, nby, nbx, 3)
    if nd.shape[1] > 1 and nd.shape[2] > 1:
        for p in range(3):
            assert (nd[..., p] == 0).any(), tag + (p, "no block without a difference")
            assert 2 * np.count_nonzero(nd[..., p]) >= nd[..., p].size, tag + (p, "fewer than half the blocks differ")


# ---- the fixtures' readers
def fixture_keys(gp):
    return sorted(k[:-3] for k in gp.files if k.endswith("_in"))


def key_parts(key):
    """'pq11_luv8_34x18_p2' -> ('pq11_luv8', 34, 18, 2)"""
    name, size, prof = key.rsplit("_", 2)
    w, h = (int(x) for x in size.split("x"))
    return name, w, h, int(prof[1])


def fixture_cases(gt):
    """(key, case, w, h, source profile) for every entry of ref_transcode.npz"""
    out = []
    for case in sorted(mg.CASES):
        for (w, h) in mg.SIZES:
            for sp in mg.SRC_PROFILES:
                k = mg.key_of(case, w, h, sp)
                assert k + "_plane0" in gt.files, k
                out.append((k, case, w, h, sp))
    return out


# ---- perturbed copies of planes
def perturbed(planes, w, h, profile):
    """a copy of three (rows, stride) uint8 planes with +-1..7 on about a tenth of the samples and a few samples of all zeros / all
    ones; the same for the same arguments; bytes beyond the sample columns are left alone"""
    rng = np.random.default_rng(w * 1000 + h * 10 + profile)
    sub, bps = profile in (0, 2), 2 if profile > 1 else 1
    out = []
    for p, pl in enumerate(planes):
        rows, cols = (h // 2, w // 2) if (p and sub) else (h, w)
        q = np.array(pl, dtype=np.uint8, copy=True)
        s = np.ascontiguousarray(q[:rows, :cols * bps])
        v = (s.view("<u2") if bps == 2 else s).astype(np.int64)
        hit = rng.random(v.shape) < 0.1
        hit[0, 0] = True
        v = np.clip(v + hit * rng.integers(1, 8, size=v.shape) * rng.choice((-1, 1), size=v.shape), 0, 0xFFFF if bps == 2 else 0xFF)
        v[rows - 1, cols - 1] = 0xFFFF if bps == 2 else 0xFF
        v[rows - 1, 0] = 0
        q[:rows, :cols * bps] = v.astype("<u2").view(np.uint8) if bps == 2 else v.astype(np.uint8)
        out.append(q)
    return out


def perturb(rng, planes, w, h, profile, frac=0.10, amp=7, extremes=3):
    """a copy of one frame's planes with +-1 .. +-amp on about `frac` of the samples and a few 0 / 0xFFFF (0xFF) samples"""
    out = []
    bps = 2 if profile > 1 else 1
    top = 0xFFFF if bps == 2 else 0xFF
    for p in range(3):
        a = np.array(planes[p], copy=True)
        rows, rb = a.shape[0], plane_rows(w, h, profile, p)[1]
        s = np.ascontiguousarray(a[:, :rb]).view("<u2" if bps == 2 else np.uint8).astype(np.int64)
        hit = rng.random(size=s.shape) < frac
        delta = rng.integers(1, amp + 1, size=s.shape) * rng.choice([-1, 1], size=s.shape)
        s = np.clip(s + hit * delta, 0, top)
        for _ in range(extremes):
            s[rng.integers(0, rows), rng.integers(0, s.shape[1])] = rng.choice([0, top])
        a[:, :rb] = s.astype("<u2" if bps == 2 else np.uint8).view(np.uint8).reshape(rows, rb)
        out.append(a)
    return out


def map_perturbed(rng, enc, ebufs, w, h, profile, block):
    """the planes a call wrote (enc: anything with .frame(bufs, f) and .nf), every frame perturbed densely (about half the samples, so
    that blocks of a few samples differ too); frame 1 keeps its rightmost block column and its bottom block row as written"""
    frames = []
    bps = 2 if profile > 1 else 1
    nbx, nby = -(-w // block), -(-h // block)
    for f in range(enc.nf):
        orig = enc.frame(ebufs, f)
        g = perturb(rng, orig, w, h, profile, frac=0.5)
        if f == 1:
            for p in range(3):
                b = block // 2 if (p and profile in (0, 2)) else block
                rb = plane_rows(w, h, profile, p)[1]
                x0, y0 = (nbx - 1) * b * bps, (nby - 1) * b
                g[p][:, x0:rb] = orig[p][:, x0:rb]
                g[p][y0:, :rb] = orig[p][y0:, :rb]
        frames.append(g)
    return frames


# ---- host buffers of the device inputs
def float_frames(rng, nf, w, h, halves=False):
    """nf (3,h,w) float32 frames: log-uniform positives with zeros, negatives and large values mixed in"""
    f = np.exp(rng.uniform(np.log(1e-4), np.log(3e4), size=(nf, 3, h, w))).astype(np.float32)
    m = rng.random(size=f.shape)
    f[m < 0.02] = 0.0
    f[(m >= 0.02) & (m < 0.04)] *= -1.0
    f[(m >= 0.04) & (m < 0.05)] = 6.5e4
    return f.astype(np.float16).astype(np.float32) if halves else f


def frames_buffer(frames, dtype=np.float32, pad=4):
    """(nf, 3 * w * h + pad) of dtype: frame f in row f, sentinel bytes in the pad behind it (frames of another float type are
    converted; frames of dtype are taken bit for bit)"""
    nf, _, h, w = frames.shape
    fs = 3 * w * h + pad
    buf = np.full(nf * fs * np.dtype(dtype).itemsize, SENTINEL, dtype=np.uint8).view(dtype).reshape(nf, fs)
    buf[:, :3 * w * h] = frames.reshape(nf, -1).astype(dtype)
    return buf


def blank_planes(w, h, profile, nf, st, gap=GAP, base=0):
    """three byte buffers of nf frames' planes behind `base` bytes, the sentinel everywhere"""
    pfs = layout(w, h, profile, st, gap)[2]
    return [np.full(base + nf * pfs[p], SENTINEL, dtype=np.uint8) for p in range(3)]


def planes_from_frames(frames, w, h, profile, st, padding, gap=GAP, base=0):
    """three byte buffers holding the given frames (lists of three (rows, >= row bytes) arrays) in rows st[p] bytes apart, the sentinel
    in every gap and in the `base` bytes in front of the first frame.  Behind each row's samples: the sentinel (padding="sentinel"), or the source rows' own bytes up to st[p]
    (padding="source"; the source rows are then at least st[p] bytes long)"""
    if padding not in ("sentinel", "source"):
        raise ValueError("padding: 'sentinel' or 'source', not %r" % (padding,))
    hs, size, pfs = layout(w, h, profile, st, gap)
    fill = blank_planes(w, h, profile, len(frames), st, gap, base)
    for f, fr in enumerate(frames):
        for p in range(3):
            n = plane_rows(w, h, profile, p)[1] if padding == "sentinel" else st[p]
            dst = fill[p][base + f * pfs[p]: base + f * pfs[p] + size[p]].reshape(hs[p], st[p])
            dst[:, :n] = np.asarray(fr[p])[:hs[p], :n]
    return fill


def random_frames(rng, w, h, profile, nf, st):
    """nf frames of three (rows, st[p]) planes: random bytes in the samples (out-of-range codes included), the sentinel behind them"""
    frames = []
    for _ in range(nf):
        fr = []
        for p in range(3):
            rows, rb = plane_rows(w, h, profile, p)
            a = np.full((rows, st[p]), SENTINEL, dtype=np.uint8)
            a[:, :rb] = rng.integers(0, 256, size=(rows, rb), dtype=np.uint8)
            fr.append(a)
        frames.append(fr)
    return frames


def gaps_intact(bufs, w, h, profile, nf, st, gap=GAP, base=0):
    """the sentinel in every gap behind a frame's plane (the last frame's too), behind every row's samples and in the `base` bytes in
    front of the first frame"""
    hs, size, pfs = layout(w, h, profile, st, gap)
    ok = True
    for p in range(3):
        ok = ok and bool(np.all(bufs[p][:base] == SENTINEL))
        b = bufs[p][base:].reshape(nf, pfs[p])
        ok = ok and bool(np.all(b[:, size[p]:] == SENTINEL))
        rb = plane_rows(w, h, profile, p)[1]
        ok = ok and bool(np.all(b[:, :size[p]].reshape(nf, hs[p], st[p])[:, :, rb:] == SENTINEL))
    return ok
