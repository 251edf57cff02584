"""Plane-to-plane measures, what needs no GPU (include/lumahip_compare.h): the six symbols are exported, declared in the new header as
lumahdrv_amd.capi's third table binds them -- header and table held to each other whatever their number, that header being the open
one -- and wrapped by Context; the header compiles as C; include/lumahip.h's closed list stands.  The numpy models the GPU test
(tests/test_gpu_planes_measure.py) holds the kernels to agree among themselves on the reference's own planes
(tests/golden/ref_planes.npz) and a perturbed copy, and the inputs that test builds (tests/support/planes_measure.py two_sets) cannot
pass a wrong kernel."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.support.device import L  # noqa: F401  (the module fixture)
from tests.support.host import BLOCKS, expected_distortion, expected_distortion_map, fixture_keys, fold_map, key_parts, perturbed
from tests.support.moments import MOM_BLOCKS, expected_moments_map, fold_2x2, sse_of
from tests.support.planes_measure import (NF, PM_DEVICE, PM_HEADER, PM_HOST, PM_METHODS, PM_SYMBOLS, case_rng, folds, inputs_cannot_pass,
                                          model, numpy_cases, swapped, two_sets)
from tests.support.tools import ROOT
from tests.support.transcode_moments import declarations, own_planes_moments

HEADER = os.path.join(ROOT, "include", PM_HEADER)


def test_the_six_symbols_are_exported_declared_and_bound(L):
    from lumahdrv_amd import capi
    table = capi._ABI_COMPARE
    assert capi.COMPARE_SYMBOLS == tuple(table) and set(PM_SYMBOLS) <= set(table)
    exported = subprocess.run(["nm", "-D", "--defined-only", capi.library_path()], capture_output=True, text=True, check=True).stdout
    for name in table:
        assert (" T " + name + "\n") in exported, name
    # header and table are the same set, whatever their number, and agree kind for kind
    decls = declarations(open(HEADER).read())
    assert sorted(decls) == sorted(table)
    scalars = {"float": C.c_float, "unsigned": C.c_uint, "int": C.c_int, "size_t": C.c_size_t}
    lib = capi.lib()
    for name, params in decls.items():
        restype, argtypes = table[name]
        assert restype is C.c_int and len(argtypes) == len(params), (name, len(argtypes), len(params))
        for k, (text, ctype) in enumerate(zip(params, argtypes)):
            if "*" in text or "[" in text:
                ok = ctype is C.c_void_p or (isinstance(ctype, type) and issubclass(ctype, C._Pointer))
            else:
                hits = [wd for wd in text.split() if wd in scalars]
                ok = len(hits) == 1 and ctype is scalars[hits[0]]
            assert ok, (name, k, text, ctype)
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == list(argtypes), name
    # the device forms share one parameter run and the host forms another; the maps add (block, words[, count])
    for names in (PM_DEVICE, PM_HOST):
        head = table[names[0]][1][:-1]
        assert all(table[n][1][:len(head)] == head for n in names), names
        assert table[names[1]][1] == table[names[2]][1] and len(table[names[1]][1]) > len(table[names[0]][1])


def test_the_set_is_disjoint_from_the_other_tables():
    from lumahdrv_amd import capi
    assert not set(capi.COMPARE_SYMBOLS) & set(capi.SYMBOLS)
    assert not set(capi.COMPARE_SYMBOLS) & set(capi.MEASURE_SYMBOLS)
    assert len(set(capi.COMPARE_SYMBOLS)) == len(capi.COMPARE_SYMBOLS)


def test_the_new_header_compiles_as_c(tmp_path):
    cc = shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler installed")
    src = tmp_path / "uses_header.c"
    src.write_text('#include "%s"\nint uses_header(void) { return (int)(%s + sizeof &lumahip_moments_map_dims) + LUMAHIP_ABI_VERSION; }\n'
                   % (PM_HEADER, " + ".join("sizeof &" + n for n in PM_SYMBOLS)))
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_closed_header_stands_and_the_methods_exist(L):
    from lumahdrv_amd import capi
    main = open(os.path.join(ROOT, "include", "lumahip.h")).read()
    decls = declarations(main)
    assert not set(PM_SYMBOLS) & set(decls) and PM_HEADER in main
    assert len(capi.SYMBOLS) == 126 and set(decls) <= set(capi.SYMBOLS)
    assert "#define LUMAHIP_ABI_VERSION 5\n" in main and capi.lib().lumahip_abi_version() == 5
    for method in PM_METHODS:
        assert callable(getattr(capi.Context, method, None)), method


def test_the_models_agree_among_themselves_on_the_reference_planes(golden_dir):
    from lumahdrv_amd import capi
    gp = np.load(os.path.join(golden_dir, "ref_planes.npz"))
    keys = fixture_keys(gp)
    assert len(keys) == 16
    for key in keys:
        name, w, h, profile = key_parts(key)
        a = [gp[key + "_plane%d" % p] for p in range(3)]
        b = perturbed(a, w, h, profile)
        frame = expected_distortion(a, b, w, h, profile)
        assert frame[:, 3].all(), key
        mom = {blk: expected_moments_map(a, b, w, h, profile, blk) for blk in MOM_BLOCKS}
        for blk in BLOCKS:
            m = expected_distortion_map(a, b, w, h, profile, blk)
            assert np.array_equal(fold_map(m), frame), (key, blk)                     # the map folds to the per-frame words
            assert m[..., 0].any() and np.array_equal(sse_of(mom[blk]), m[..., 0]), (key, blk)   # See - 2 Seg + Sgg is the map's sse
        for blk in MOM_BLOCKS[:-1]:
            assert np.array_equal(fold_2x2(mom[blk]), mom[2 * blk]), (key, blk)        # 2 x 2 moment blocks add up
        # A against itself: no difference anywhere, Se == Sg, See == Sgg == Seg, and a structural similarity of exactly 1
        assert not expected_distortion(a, a, w, h, profile).any(), key
        for blk in MOM_BLOCKS:
            own = expected_moments_map(a, a, w, h, profile, blk)
            assert own_planes_moments(own) and not own_planes_moments(mom[blk]), (key, blk)
            counts = capi.moments_sample_counts(w, h, profile, blk)
            for p in range(3):
                peak = float((1 << (16 if profile > 1 else 8)) - 1)
                assert np.all(capi.code_ssim(own[:, :, p], counts[:, :, p], peak) == 1.0), (key, blk, p)
            # exchanging the sets exchanges words 0 <-> 1 and 2 <-> 3 and leaves the cross moment
            assert np.array_equal(expected_moments_map(b, a, w, h, profile, blk), swapped(mom[blk])), (key, blk)
            assert not np.array_equal(swapped(mom[blk]), mom[blk]), (key, blk)


def test_the_gpu_tests_inputs_cannot_pass_a_wrong_kernel():
    """every profile x size of the GPU test against numpy, as that test builds them"""
    cases = numpy_cases()
    assert len(cases) == 24
    many = 0
    for profile, w, h in cases:
        a, b, st = two_sets(case_rng(profile, w, h), w, h, profile)
        assert len(a) == len(b) == NF
        frame, maps, moms = model(a, b, w, h, profile)
        tag = (profile, w, h)
        inputs_cannot_pass(frame, maps, moms, tag)
        folds(frame, maps, moms, tag)
        many += sum(m.shape[1] > 1 and m.shape[2] > 1 for m in list(maps.values()) + list(moms.values()))
        # the three frames are distinct, and the bytes behind the samples are the same in both sets
        assert not np.array_equal(frame[0], frame[1]) and not np.array_equal(frame[1], frame[2]), tag
        for f in range(NF):
            for p in range(3):
                rb = st[p] - 5
                assert np.array_equal(a[f][p][:, rb:], b[f][p][:, rb:]), tag
        # the swap the GPU test relies on
        sw = model(b, a, w, h, profile)
        assert np.array_equal(sw[0], frame), tag
        for blk in MOM_BLOCKS:
            assert np.array_equal(sw[2][blk], swapped(moms[blk])) and not np.array_equal(sw[2][blk], moms[blk]), tag + (blk,)
    assert many >= 4 * 7   # (34, 18) at 8 and 16, (264, 70) at every block: maps with more than one row and column
