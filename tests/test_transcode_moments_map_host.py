"""Transcode moments map, what needs no GPU (include/lumahip_measure.h lumahip_transcode_moments_map_frames_device / _frame_host):
the two symbols are exported, declared in the new header as lumahdrv_amd.capi's second table binds them, and wrapped by Context; the
header compiles as C; the numpy model the GPU test holds the kernels to (tests/support/moments.py expected_moments_map) is tied to the
distortion map's model and to itself across block sizes on the reference's own decode -> encode (tests/golden/ref_transcode.npz);
and the inputs the GPU test builds (tests/support/transcode_moments.py given_frames) cannot pass a wrong kernel.

given_frames is tests/support/host.py map_perturbed with two amendments, because map_perturbed alone cannot give Seg != See in every
plane of every frame: where a map has one block column or row, its frame 1 -- which keeps the rightmost block column and the bottom
block row as written -- is the written frame itself."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.golden import make_transcode_golden as mg
from tests.support.device import L  # noqa: F401  (the module fixture)
from tests.support.host import BLOCKS, expected_distortion_map, fixture_cases, perturbed, plane_rows, random_frames
from tests.support.moments import MOM_BLOCKS, expect_moments, expected_moments_map, fold_2x2, sse_of
from tests.support.tools import ROOT
from tests.support.transcode_moments import (TMOM_HEADER, TMOM_SYMBOLS, HostPlanes, blocks_at, declarations, given_frames,
                                             inputs_cannot_pass_a_wrong_kernel, kept_block, own_planes_moments, pairs_cases)

HEADER = os.path.join(ROOT, "include", TMOM_HEADER)


def test_both_symbols_are_exported_and_bound(L):
    from lumahdrv_amd import capi
    exported = subprocess.run(["nm", "-D", "--defined-only", capi.library_path()], capture_output=True, text=True, check=True).stdout
    for name in TMOM_SYMBOLS:
        assert (" T " + name + "\n") in exported, name
    assert list(capi.MEASURE_SYMBOLS) == TMOM_SYMBOLS and capi.MEASURE_SYMBOLS == tuple(capi._ABI_MEASURE)
    assert not set(capi.MEASURE_SYMBOLS) & set(capi.SYMBOLS)
    lib = capi.lib()
    for name in TMOM_SYMBOLS:
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == list(capi._ABI_MEASURE[name][1]), name
    assert lib.lumahip_abi_version() == 5
    for method in ("transcode_moments_map_frames_device", "transcode_moments_map_frame"):
        assert callable(getattr(capi.Context, method, None)), method


def test_the_new_header_declares_what_the_second_table_binds():
    from lumahdrv_amd import capi
    decls = declarations(open(HEADER).read())
    assert sorted(decls) == sorted(TMOM_SYMBOLS)
    scalars = {"float": C.c_float, "unsigned": C.c_uint, "int": C.c_int, "size_t": C.c_size_t}
    for name, params in decls.items():
        restype, argtypes = capi._ABI_MEASURE[name]
        assert restype is C.c_int and len(argtypes) == len(params), (name, len(argtypes), len(params))
        for k, (text, ctype) in enumerate(zip(params, argtypes)):
            if "*" in text or "[" in text:
                ok = ctype is C.c_void_p or (isinstance(ctype, type) and issubclass(ctype, C._Pointer))
            else:
                hits = [wd for wd in text.split() if wd in scalars]
                ok = len(hits) == 1 and ctype is scalars[hits[0]]
            assert ok, (name, k, text, ctype)
    # ... and they are the transcode distortion map calls' parameters, kind for kind
    for name in TMOM_SYMBOLS:
        assert capi._ABI_MEASURE[name] == capi._ABI[name.replace("moments_map", "distortion_map")], name
    # lumahip.h itself declares neither (its list of declarations is closed), only names them in its ABI history
    main = open(os.path.join(ROOT, "include", "lumahip.h")).read()
    assert not set(TMOM_SYMBOLS) & set(declarations(main))
    assert all(name in main for name in TMOM_SYMBOLS) and TMOM_HEADER in main


def test_the_new_header_compiles_as_c(tmp_path):
    cc = shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler installed")
    src = tmp_path / "uses_header.c"
    src.write_text('#include "%s"\nint uses_header(void) { return (int)(sizeof &lumahip_transcode_moments_map_frames_device +\n'
                   '    sizeof &lumahip_transcode_moments_map_frame_host + sizeof &lumahip_moments_map_dims) + LUMAHIP_ABI_VERSION; }\n' % TMOM_HEADER)
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_model_on_the_reference_fixture(L, golden_dir):
    from lumahdrv_amd import capi
    gt = np.load(os.path.join(golden_dir, "ref_transcode.npz"))
    n = 0
    for k, case, w, h, sp in fixture_cases(gt):
        fix = [gt[k + "_plane%d" % p] for p in range(3)]
        bad = perturbed(fix, w, h, mg.DST_PROFILE)
        got, own = {}, {}
        for block in MOM_BLOCKS:
            nbx, nby = -(-w // block), -(-h // block)
            got[block] = expected_moments_map(fix, bad, w, h, mg.DST_PROFILE, block)
            assert got[block].shape == (nby, nbx, 3, 5) and got[block].dtype == np.uint64, (k, block)
            own[block] = expected_moments_map(fix, fix, w, h, mg.DST_PROFILE, block)
            assert own_planes_moments(own[block]), (k, block)
            counts = capi.moments_sample_counts(w, h, mg.DST_PROFILE, block)
            assert counts.shape == (nby, nbx, 3)
            dname = mg.CASES[case][2]
            peaks = np.array([(1 << mg.CONFIGS[dname][1]) - 1] + 2 * [(1 << mg.CONFIGS[dname][3]) - 1], dtype=np.float64)
            for p in range(3):
                ssim = capi.code_ssim(own[block][:, :, p], counts[:, :, p], peaks[p])
                assert ssim.shape == (nby, nbx) and np.all(ssim == 1.0), (k, block, p, ssim)
                other = capi.code_ssim(got[block][:, :, p], counts[:, :, p], peaks[p])
                assert np.all(other <= 1.0) and np.any(other < 1.0), (k, block, p, other)
        for block in BLOCKS:
            sse = expected_distortion_map(fix, bad, w, h, mg.DST_PROFILE, block)[..., 0]
            assert sse.any() and np.array_equal(sse_of(got[block]), sse), (k, block)
            assert not sse_of(own[block]).any(), (k, block)
        for block in (8, 16, 32):
            assert np.array_equal(fold_2x2(got[block]), got[2 * block]), (k, block)
        n += 1
    assert n == 16


def test_the_gpu_tests_inputs_cannot_pass_a_wrong_kernel():
    """random planes stand in for e: every size x target profile x block of the GPU test's pairs test"""
    rng = np.random.default_rng(2024)
    n = many = 0
    for it, sp, dp, w, h in pairs_cases():
        st = tuple(plane_rows(w, h, dp, p)[1] + 5 for p in range(3))
        frames = random_frames(rng, w, h, dp, 3, st)
        enc = HostPlanes(frames, w, h, dp)
        blocks = blocks_at(w, h, it)
        given = HostPlanes(given_frames(rng, enc, frames, w, h, dp, kept_block(w, h, blocks)), w, h, dp)
        # the paddings behind the samples are as they were
        for f in range(3):
            for p in range(3):
                rb = plane_rows(w, h, dp, p)[1]
                assert np.array_equal(given.frames[f][p][:, rb:], frames[f][p][:, rb:])
        for block in blocks:
            exp = expect_moments(enc, frames, given, given.frames, block)
            inputs_cannot_pass_a_wrong_kernel(exp, (sp, dp, w, h, block))
            many += exp.shape[1] > 1 and exp.shape[2] > 1
            n += 1
    assert n == 16 * (2 * 4 + 4) and many >= 16 * 5, (n, many)
    # a kernel that took e for g (or g for e) is caught: its map would be that of planes against themselves
    assert not own_planes_moments(exp)
