"""Transcode distortion without a GPU: the exported symbols, and the numpy expectation the GPU test
(tests/test_gpu_transcode_distortion.py) holds the kernels to -- checked here on the reference's own transcoded planes in
tests/golden/ref_transcode.npz: zeros against themselves, something else than zeros against a deterministically perturbed copy,
for every key (so that the fixture cases of the GPU test are not vacuous)."""
import os

import numpy as np

from tests.golden import make_transcode_golden as mg
from tests.support.host import expected_distortion, fixture_cases, perturbed

SYMBOLS = ["lumahip_transcode_distortion_frames_device", "lumahip_transcode_distortion_frame_host"]


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
