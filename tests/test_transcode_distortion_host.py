"""Transcode distortion without a GPU: the exported symbols, and the numpy expectation the GPU test
(tests/test_gpu_transcode_distortion.py) holds the kernels to -- checked here on the reference's own transcoded planes in
tests/golden/ref_transcode.npz: zeros against themselves, something else than zeros against a deterministically perturbed copy,
for every key (so that the fixture cases of the GPU test are not vacuous)."""
import os

import numpy as np

from tests.golden import make_transcode_golden as mg
from tests.test_distortion_host import expected_distortion

SYMBOLS = ["lumahip_transcode_distortion_frames_device", "lumahip_transcode_distortion_frame_host"]


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


def test_library_exports_the_transcode_distortion_symbols():
    from lumahdrv_amd import capi
    L = capi.lib()
    for s in SYMBOLS:
        assert s in capi.SYMBOLS and hasattr(L, s), s
    assert L.lumahip_abi_version() == 5


def test_expectation_is_zero_on_the_fixture_against_itself_and_not_on_a_perturbed_copy(golden_dir):
    gt = np.load(os.path.join(golden_dir, "ref_transcode.npz"))
    cases = fixture_cases(gt)
    assert len(cases) == 16 and len(cases) == sum(k.endswith("_stride") for k in gt.files)
    for k, _, w, h, _ in cases:
        pl = [gt[k + "_plane%d" % p] for p in range(3)]
        assert not expected_distortion(pl, pl, w, h, mg.DST_PROFILE).any(), k
        bad = perturbed(pl, w, h, mg.DST_PROFILE)
        e = expected_distortion(pl, bad, w, h, mg.DST_PROFILE)
        assert e[:, 3].all(), k                     # every plane differs somewhere
        assert np.all(e[:, 0] >= e[:, 1]) and np.all(e[:, 1] >= e[:, 2]) and np.all(e[:, 1] >= e[:, 3]), k
        assert np.array_equal(e, expected_distortion(pl, perturbed(pl, w, h, mg.DST_PROFILE), w, h, mg.DST_PROFILE)), k
        for p in range(3):                           # the bytes beyond the samples are the fixture's
            rb = (w // 2 if p else w) * 2
            assert np.array_equal(bad[p][:, rb:], pl[p][:, rb:]), k
