"""The transcode distortion map without a GPU: the exported symbols and the Context methods, and the numpy expectation the GPU test
(tests/test_gpu_transcode_distortion_map.py) holds the kernels to -- checked here on the reference's own transcoded planes in
tests/golden/ref_transcode.npz: for every key and block size the map of the fixture against a deterministically perturbed copy folds
to the per-frame expectation of the same pair and is not zero, and the map of the fixture against itself is."""
import os
import re

import numpy as np

from tests.golden import make_transcode_golden as mg
from tests.support.host import BLOCKS, expected_distortion, expected_distortion_map, fixture_cases, fold_map, perturbed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["lumahip_transcode_distortion_map_frames_device", "lumahip_transcode_distortion_map_frame_host"]


def test_library_exports_the_transcode_distortion_map_symbols():
    from lumahdrv_amd import capi
    L = capi.lib()
    with open(os.path.join(ROOT, "include", "lumahip.h")) as fh:
        header = fh.read()
    for s in SYMBOLS:
        assert re.search(r"\bint %s\(" % s, header), s + " is not declared in the header"
        assert s in capi.SYMBOLS and hasattr(L, s), s
    assert L.lumahip_abi_version() == 5
    assert callable(getattr(capi.Context, "transcode_distortion_map_frames_device", None))
    assert callable(getattr(capi.Context, "transcode_distortion_map_frame", None))


def test_expected_map_folds_to_the_frame_expectation_on_the_transcode_fixture(golden_dir):
    gt = np.load(os.path.join(golden_dir, "ref_transcode.npz"))
    cases = fixture_cases(gt)
    assert len(cases) == 16
    for k, _, w, h, _ in cases:
        pl = [gt[k + "_plane%d" % p] for p in range(3)]
        bad = perturbed(pl, w, h, mg.DST_PROFILE)
        frame = expected_distortion(pl, bad, w, h, mg.DST_PROFILE)
        for block in BLOCKS:
            m = expected_distortion_map(pl, bad, w, h, mg.DST_PROFILE, block)
            assert m.shape == (-(-h // block), -(-w // block), 3, 4) and m.dtype == np.uint64
            assert m.any() and np.array_equal(fold_map(m), frame), (k, block)
            assert not expected_distortion_map(pl, pl, w, h, mg.DST_PROFILE, block).any(), (k, block)
