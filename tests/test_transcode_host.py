"""Re-quantizing code planes without a GPU: the oracle's decode followed by its encode reproduces tests/golden/ref_transcode.npz
(the reference's own decode -> encode of the `_dec_plane*` planes of ref_planes.npz, tests/golden/make_transcode_golden.py) bit
for bit.  The fused GPU call is held to the same fixture in tests/test_gpu_transcode.py."""
import os

import numpy as np
import pytest

from tests.golden.make_transcode_golden import CASES, CONFIGS, DST_PROFILE, SIZES, SRC_PROFILES, key_of, source_planes, transcode


def row_bytes(w, h, profile, p):
    sub, bps = profile in (0, 2), 2 if profile > 1 else 1
    return ((w + 1) // 2 if (p and sub) else w) * bps


def test_fixture_holds_every_case(golden_dir):
    gt = np.load(os.path.join(golden_dir, "ref_transcode.npz"))
    want = {key_of(c, w, h, sp) + s for c in CASES for (w, h) in SIZES for sp in SRC_PROFILES for s in ("_plane0", "_plane1", "_plane2", "_stride")}
    assert want | {"cases"} == set(gt.files)
    assert os.path.getsize(os.path.join(golden_dir, "ref_transcode.npz")) < 256 * 1024


@pytest.mark.parametrize("case", sorted(CASES))
def test_oracle_decode_then_encode_equals_the_reference(oracle_mod, golden_dir, case):
    o = oracle_mod
    gp = np.load(os.path.join(golden_dir, "ref_planes.npz"))
    gt = np.load(os.path.join(golden_dir, "ref_transcode.npz"))
    src, src_sc, dst, dst_sc = CASES[case]
    dec, enc = o.Oracle(*CONFIGS[src]), o.Oracle(*CONFIGS[dst])
    for (w, h) in SIZES:
        for sp in SRC_PROFILES:
            planes, st = source_planes(gp, src, w, h, sp)
            got, gst = transcode(dec, enc, planes, st, w, h, src_sc, sp, dst_sc, DST_PROFILE)
            k = key_of(case, w, h, sp)
            assert tuple(gst) == tuple(int(s) for s in gt[k + "_stride"]), k
            for p in range(3):
                n = row_bytes(w, h, DST_PROFILE, p)   # (beyond the row: the reference harness's fill, never written)
                assert np.array_equal(got[p][:, :n], gt[k + "_plane%d" % p][:, :n]), (k, p)
