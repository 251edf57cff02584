"""The moments map without a GPU: the exported symbols, lumahip_moments_map_dims, moments_sample_counts, code_ssim, and the numpy
expectation the GPU test (tests/test_gpu_moments_map.py) holds the kernels to (tests/support/moments.py) -- checked here against
itself across block sizes and against the distortion map's expectation on the reference's own planes in tests/golden/ref_planes.npz,
and on a hand-made case that pins which block a 4:2:0 chroma sample belongs to."""
import ctypes as C
import os
from fractions import Fraction

import numpy as np
import pytest

from tests.support.host import BLOCKS, expected_distortion_map, fixture_keys, key_parts
from tests.support.moments import MOM_BLOCKS, MOM_SYMBOLS, expected_moments_map, fold_2x2, sse_of


def test_library_exports_the_moments_symbols():
    from lumahdrv_amd import capi
    L = capi.lib()
    for s in MOM_SYMBOLS:
        assert s in capi.SYMBOLS and hasattr(L, s), s
    assert L.lumahip_abi_version() == 5
    for m in ("moments_map_frames_device", "moments_map_frames_device_planar", "moments_map_frames_device_f16",
              "moments_map_frames_device_planar_f16", "moments_map_frame"):
        assert callable(getattr(capi.Context, m)), m


def test_moments_map_dims():
    import lumahdrv_amd
    from lumahdrv_amd import capi
    assert lumahdrv_amd.moments_map_dims(34, 18, 8) == (5, 3)
    assert capi.moments_map_dims(3840, 2160, 8) == (480, 270)
    assert capi.moments_map_dims(3840, 2160, 64) == capi.distortion_map_dims(3840, 2160, 64) == (60, 34)
    L = capi.lib()
    for block in (0, 4, 48, 128):
        nbx, nby = C.c_uint(77), C.c_uint(77)
        assert L.lumahip_moments_map_dims(64, 64, block, C.byref(nbx), C.byref(nby)) == capi.ERR_ARG, block
        assert (nbx.value, nby.value) == (77, 77)
        with pytest.raises(capi.LumaHipError):
            capi.moments_map_dims(64, 64, block)
    # the distortion map keeps refusing blocks of 8
    with pytest.raises(capi.LumaHipError):
        capi.distortion_map_dims(64, 64, 8)
    with pytest.raises(capi.LumaHipError):
        capi.block_sample_counts(64, 64, 2, 8)


def test_expected_moments_fold_across_block_sizes_and_to_the_distortion_map(golden_dir):
    gp = np.load(os.path.join(golden_dir, "ref_planes.npz"))
    keys = fixture_keys(gp)
    assert len(keys) == 16
    for key in keys:
        _, w, h, profile = key_parts(key)
        pl = [gp[key + "_plane%d" % p] for p in range(3)]
        dpl = [gp[key + "_dec_plane%d" % p] for p in range(3)]
        maps = {b: expected_moments_map(pl, dpl, w, h, profile, b) for b in MOM_BLOCKS}
        for b in MOM_BLOCKS:
            assert maps[b].shape == (-(-h // b), -(-w // b), 3, 5) and maps[b].dtype == np.uint64
        for b in (8, 16, 32):     # ragged edges included: 2 x 2 blocks, or what there is of them
            assert np.array_equal(fold_2x2(maps[b]), maps[2 * b]), (key, b)
        for b in BLOCKS:
            d = expected_distortion_map(pl, dpl, w, h, profile, b)
            assert d[..., 0].any() and np.array_equal(sse_of(maps[b]), d[..., 0]), (key, b)
        own = expected_moments_map(pl, pl, w, h, profile, 8)
        assert np.array_equal(own[..., 0], own[..., 1]) and np.array_equal(own[..., 2], own[..., 3]) and np.array_equal(own[..., 2], own[..., 4])


def test_expected_moments_put_chroma_samples_into_their_blocks():
    # 40 x 36 pixels, 4:2:0, 16-bit, blocks of 16: 3 x 3 blocks; the chroma planes are 20 x 18 samples in blocks of 8
    w, h = 40, 36
    ya = np.full((h + 2, 2 * w + 6), 0xC3, dtype=np.uint8)
    ca = np.full((h // 2 + 2, w + 6), 0xC3, dtype=np.uint8)
    ya[:h, :2 * w] = 0
    ca[:h // 2, :w] = 0
    ye, ue = ya.copy(), ca.copy()
    ye[17, 2 * 33] = 3                                    # e: luma pixel (x 33, y 17) = 3
    ue[7, 2 * 8] = 7                                      # e: U sample (x 8, y 7) = 7
    yb, ub, vb = ya.copy(), ca.copy(), ca.copy()
    yb[17, 2 * 33], yb[17, 2 * 33 + 1] = 0x34, 0x12      # g: luma pixel (x 33, y 17) = 0x1234: block (2, 1)
    ub[7, 2 * 8] = 5                                     # U sample (x 8, y 7): co-sited with luma (16..17, 14..15): block (1, 0)
    ub[8, 2 * 7] = 3                                     # U sample (x 7, y 8): block (0, 1)
    vb[17, 2 * 19], vb[17, 2 * 19 + 1] = 2, 1            # V sample (x 19, y 17) = 0x0102: the last one, block (2, 2)
    yb[h, 0] = yb[0, 2 * w] = ub[h // 2, 0] = ub[0, w] = vb[0, w + 1] = 1   # bytes outside the samples do not count
    m = expected_moments_map([ye, ue, ca], [yb, ub, vb], w, h, 2, 16)
    want = np.zeros((3, 3, 3, 5), dtype=np.uint64)
    want[1, 2, 0] = (3, 0x1234, 9, 0x1234 ** 2, 3 * 0x1234)
    want[0, 1, 1] = (7, 5, 49, 25, 35)
    want[1, 0, 1] = (0, 3, 0, 9, 0)
    want[2, 2, 2] = (0, 0x0102, 0, 0x0102 ** 2, 0)
    assert m.shape == (3, 3, 3, 5) and np.array_equal(m, want)
    # blocks of 8 (chroma: 4): 5 x 5 blocks
    m8 = expected_moments_map([ye, ue, ca], [yb, ub, vb], w, h, 2, 8)
    want8 = np.zeros((5, 5, 3, 5), dtype=np.uint64)
    want8[2, 4, 0] = want[1, 2, 0]
    want8[1, 2, 1] = want[0, 1, 1]
    want8[2, 1, 1] = want[1, 0, 1]
    want8[4, 4, 2] = want[2, 2, 2]
    assert np.array_equal(m8, want8)
    # 4:4:4 (profile 3): the same bytes are chroma samples of full-size blocks
    m3 = expected_moments_map([ye, ya, ye], [yb, ya, yb], w, h, 3, 16)
    assert m3[1, 2, 0].tolist() == m3[1, 2, 2].tolist() == [3, 0x1234, 9, 0x1234 ** 2, 3 * 0x1234] and not m3[:, :, 1].any()
    assert int(np.count_nonzero(m3[:, :, :, 1])) == 2


def test_moments_sample_counts():
    from lumahdrv_amd import block_sample_counts, moments_sample_counts
    for w, h in ((34, 18), (64, 32), (264, 70), (6, 4)):
        for profile in range(4):
            for block in MOM_BLOCKS:
                n = moments_sample_counts(w, h, profile, block)
                assert n.shape == (-(-h // block), -(-w // block), 3) and n.dtype == np.int64
                cw, ch = (w // 2, h // 2) if profile in (0, 2) else (w, h)
                assert n.sum(axis=(0, 1)).tolist() == [w * h, cw * ch, cw * ch]
                assert (n > 0).all()
                if block in BLOCKS:
                    assert np.array_equal(n, block_sample_counts(w, h, profile, block))
    # 34 x 18 in blocks of 8: columns of 8, 8, 8, 8, 2 pixels, rows of 8, 8, 2
    n = moments_sample_counts(34, 18, 2, 8)
    assert n[:, :, 0].tolist() == [[64, 64, 64, 64, 16], [64, 64, 64, 64, 16], [16, 16, 16, 16, 4]]
    assert n[:, :, 1].tolist() == n[:, :, 2].tolist() == [[16, 16, 16, 16, 4], [16, 16, 16, 16, 4], [4, 4, 4, 4, 1]]


def _ssim_fraction(e, g, peak, k1, k2):
    """the formula of code_ssim's docstring over two lists of integers, in rationals"""
    n = len(e)
    se, sg = sum(e), sum(g)
    see, sgg, seg = sum(x * x for x in e), sum(x * x for x in g), sum(x * y for x, y in zip(e, g))
    c1, c2 = (Fraction(str(k1)) * peak) ** 2, (Fraction(str(k2)) * peak) ** 2
    return ((2 * se * sg + n * n * c1) * (2 * (n * seg - se * sg) + n * n * c2) /
            ((se * se + sg * sg + n * n * c1) * ((n * see - se * se) + (n * sgg - sg * sg) + n * n * c2)))


def _moments(e, g):
    return np.array([sum(e), sum(g), sum(x * x for x in e), sum(x * x for x in g), sum(x * y for x, y in zip(e, g))], dtype=np.uint64)


# fewer than 20 rounded float64 operations behind the exact integer parts, each within 1.1e-16
SSIM_RTOL = 1e-12


def test_code_ssim(golden_dir):
    from lumahdrv_amd import code_ssim, moments_sample_counts
    # identical planes: exactly 1.0, whatever they hold
    gp = np.load(os.path.join(golden_dir, "ref_planes.npz"))
    for key in fixture_keys(gp):
        _, w, h, profile = key_parts(key)
        pl = [gp[key + "_plane%d" % p] for p in range(3)]
        for block in (8, 64):
            m = expected_moments_map(pl, pl, w, h, profile, block)
            s = code_ssim(m, moments_sample_counts(w, h, profile, block), 0xFFFF if profile > 1 else 0xFF)
            assert s.dtype == np.float64 and s.shape == m.shape[:-1] and np.all(s == 1.0), (key, block)
    # a hand-made 2 x 2 window
    e, g = [10, 20, 30, 40], [12, 18, 33, 41]
    got = code_ssim(_moments(e, g), np.int64(4), 255)
    want = _ssim_fraction(e, g, 255, 0.01, 0.03)
    assert got.shape == () and abs(Fraction(float(got)) - want) <= SSIM_RTOL * want, (float(got), float(want))
    assert 0.9 < float(got) < 1.0
    # N See and Se^2 agree in their top 40 bits and more (2^55.7 both, 4095 apart): the difference is formed in integers.  With small
    # constants the quotient hangs on it -- rounded to float64 first, N See alone would be off by up to 4 and the result by 1e-3
    n = 4096
    e, g = [60000] * n, [60000] * n
    e[5], g[77] = 60001, 59999
    me = _moments(e, g)
    a, b = n * int(me[2]), int(me[0]) ** 2
    assert a.bit_length() == b.bit_length() == 56 and a - b == 4095 < 1 << (56 - 40)
    got = code_ssim(me[None], np.array([n]), 0xFFFF, k1=1e-9, k2=1e-9)
    want = _ssim_fraction(e, g, 0xFFFF, 1e-9, 1e-9)
    assert abs(Fraction(float(got[0])) - want) <= SSIM_RTOL * want, (float(got[0]), float(want))
    assert 2e-4 < float(got[0]) < 3e-4          # (2 + c) / (8190 + c)
    # constant planes of different level: zero variances, the luminance term alone
    e, g = [100] * 64, [120] * 64
    got = code_ssim(_moments(e, g), 64, 255)
    want = _ssim_fraction(e, g, 255, 0.01, 0.03)
    assert want == Fraction(2 * 100 * 120 * 10000 + 255 * 255, (100 * 100 + 120 * 120) * 10000 + 255 * 255)
    assert abs(Fraction(float(got)) - want) <= SSIM_RTOL * want, (float(got), float(want))
    # arguments
    with pytest.raises(ValueError):
        code_ssim(np.zeros((2, 4), dtype=np.uint64), np.ones(2), 255)
    with pytest.raises(ValueError):
        code_ssim(np.zeros((2, 5), dtype=np.uint64), np.ones(3), 255)
    with pytest.raises(ValueError):
        code_ssim(np.zeros((2, 5), dtype=np.uint64), np.zeros(2), 255)
