"""What tests/test_gpu_measuring_kernels.py relies on, checked without a GPU: the measuring matrix names the 216 frame-fed measuring
kernels its docstring says -- 72 each of k_distortion, k_distortion_map and k_moments_map -- every call form and block size meets every
colour space, and the inputs of every row can tell a wrong kernel from a right one: the oracle's planes are informative, the given
planes differ from them in every plane of every frame, no map is all zeros or all differences, the three frames of a launch have
different words, and the 264x70 frames hold NaN, both infinities and negatives."""
import numpy as np

from tests.support import frame_kernels as fk
from tests.support import measuring as ms
from tests.support.host import BLOCKS, SENTINEL, gaps_intact, neither_path_is_vacuous, widen_halves
from tests.support.moments import MOM_BLOCKS, sse_of

ROWS = ms.measuring_matrix()


def test_the_matrix_covers_what_the_docstring_says():
    """per family 72 k_*<CS, SUB, VW, LM, IN16>: RGB, XYZ and Lu'v' with LM 3 and 7 by SUB, VW 4 and 2, float and binary16 frames (48);
    YCbCr float frames with LM 5, 3 and 7 (12); YCbCr binary16 frames with LM 6, 3 and 7 (12)"""
    assert len({r.id for r in ROWS}) == len(ROWS)
    kernels = {ms.kernel_of(r) for r in ROWS}
    print("%d distinct kernels: %s" % (len(kernels), ", ".join("%d %s" % (sum(k[0] == f for k in kernels), f) for f in ms.FAMILIES)))
    assert len(kernels) == 216
    subs_vws = [(sub, vw) for sub in (True, False) for vw in (4, 2)]
    for family in ms.FAMILIES:
        mine = {k[1:] for k in kernels if k[0] == family}
        assert len(mine) == 72
        plain = {(cs, sub, vw, lm, in16) for cs in (fk.LUV, fk.RGB, fk.XYZ) for (sub, vw) in subs_vws for lm in (3, 7) for in16 in (False, True)}
        yf = {(fk.YCC, sub, vw, lm, False) for (sub, vw) in subs_vws for lm in (5, 3, 7)}
        yh = {(fk.YCC, sub, vw, lm, True) for (sub, vw) in subs_vws for lm in (6, 3, 7)}
        assert (len(plain), len(yf), len(yh)) == (48, 12, 12) and mine == plain | yf | yh
    for family in ms.FAMILIES:
        for cs in fk.SPACES:
            rows = [r for r in ROWS if r.family == family and r.cs == cs]
            # every call form, and both preScalings of YCbCr, on every front end
            assert {r.form for r in rows} == set(ms.FLOAT_FORMS + ms.HALF_FORMS), (family, cs)
            assert {(r.lm, r.in16, r.form) for r in rows if r.cfg[1] != 8} == \
                {(lm, in16, form) for in16 in (False, True) for (lm, _, _) in ms.contexts_of(cs, in16)
                 for form in (ms.HALF_FORMS if in16 else ms.FLOAT_FORMS)}, (family, cs)
            assert {r.sc for r in rows} == set(fk.SPACES[cs][4])
            # the 8-bit profiles, both frame types, four and two pixels per thread
            assert {(r.profile, r.in16) for r in rows if r.profile < 2} == {(p, i) for p in (0, 1) for i in (False, True)}, (family, cs)
            assert {(r.in16, r.w) for r in rows if r.profile < 2} == {(i, w) for i in (False, True) for w in (264, 258)}, (family, cs)
            # every block size on the size with several block columns and rows, and on the four-pixel kernels of both frame types
            blocks = {"distortion": {None}, "distortion_map": set(BLOCKS), "moments_map": set(MOM_BLOCKS)}[family]
            for in16 in (False, True):
                assert {r.block for r in rows if (r.w, r.h) == (264, 70) and r.in16 == in16} == blocks, (family, cs, in16)
    # which front end a YCbCr context is expected to report
    assert {(r.lm, r.in16, ms.half_table_used(r)) for r in ROWS if r.cs == fk.YCC and r.cfg[1] != 8} == \
        {(5, False, True), (6, True, True), (3, False, False), (3, True, False), (7, False, False), (7, True, False)}


def test_the_frames_hold_the_special_values():
    for (w, h) in ms.SIZES:
        f = fk.frames(w, h)
        big = (w, h) == (264, 70)
        assert np.isnan(f).any() == big and np.isposinf(f).any() == big and np.isneginf(f).any() == big and bool((f < 0).any()) == big
        h16 = widen_halves(fk.frames(w, h, halves=True))
        assert np.isnan(h16).any() == big and np.isposinf(h16).any() == big and np.isneginf(h16).any() == big and bool((h16 < 0).any()) == big


def test_the_oracles_planes_are_informative(oracle_mod):
    """at least 64 distinct sample values in every plane the oracle writes for a row's frames at 264x70 and 258x6, U and V different"""
    keys = sorted({(r.cfg, r.profile, r.w, r.h, r.sc, r.in16) for r in ROWS if (r.w, r.h) != (6, 4)})
    least = min(fk.informative(fk.expected(oracle_mod, *k)[1], k[2], k[3], k[1], k) for k in keys)
    print("%d reference launches; the fewest distinct sample values of an expected plane: %d" % (len(keys), least))
    assert least >= fk.MIN_DISTINCT


def test_every_row_can_tell_a_wrong_kernel(oracle_mod):
    """the conditions on the inputs, asserted on the reference alone"""
    least = None
    for r in ROWS:
        gv = ms.given_of(oracle_mod, r)
        nd = gv.dist[:, :, 3]
        assert (nd > 0).all(), (r.id, "a plane of a frame without a difference", nd)
        least = int(nd.min()) if least is None else min(least, int(nd.min()))
        for a in range(fk.NF):
            for b in range(a + 1, fk.NF):
                assert not np.array_equal(gv.words[a], gv.words[b]), (r.id, a, b, "two frames with the same words")
        if r.family != "distortion":
            neither_path_is_vacuous(gv.dmap, (r.id,))
            nby, nbx = -(-r.h // r.block), -(-r.w // r.block)
            assert gv.words.shape == (fk.NF, nby, nbx, 3, 4 if r.family == "distortion_map" else 5), r.id
        if r.family == "moments_map":   # (the two numpy models agree on what they share)
            assert np.array_equal(sse_of(gv.words), gv.dmap[..., 0]), r.id
        # the same samples whatever the layout, and the sentinel around them
        for hp in (ms.HostPlanes(gv.g, r.w, r.h, r.profile), ms.HostPlanes(gv.g, r.w, r.h, r.profile, *fk.odd_layout(r.w, r.h, r.profile), base=1)):
            assert gaps_intact(hp.bufs, r.w, r.h, r.profile, fk.NF, hp.st, hp.gap, hp.base) and (hp.bufs[0][:hp.base] == SENTINEL).all(), r.id
            assert fk.planes_problem(hp.bufs, gv.g, r.w, r.h, r.profile, hp.st, hp.gap, hp.base) is None, r.id
    print("%d rows; the smallest n_differ of a plane of a frame: %d" % (len(ROWS), least))


def test_the_layouts_are_what_their_names_say():
    for profile in range(4):
        for (w, h) in ms.SIZES[:2]:
            st, gap = fk.odd_layout(w, h, profile)
            hp = ms.HostPlanes([], w, h, profile, st, gap, base=1)
            assert all(s % 2 == 1 for s in hp.st) and all(x % 2 == 1 for x in hp.pfs)
        st, base = ms.half_aligned_layout(264, 70, profile)
        hp = ms.HostPlanes([], 264, 70, profile, st, base=base)
        unit = 8 if profile > 1 else 4       # four samples
        assert base % unit == unit // 2 and all(s % 8 == 0 for s in hp.st) and all(x % 8 == 0 for x in hp.pfs)
