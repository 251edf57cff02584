"""What tests/test_gpu_plane_kernels.py relies on, checked without a GPU: the plane matrix names the 192 plane-fed kernels its docstring
says -- 48 each of k_transcode, k_transcode_distortion, k_transcode_distortion_map and k_transcode_moments_map -- every block size
meets every pair, every YCbCr-source kernel runs with and without the short division by its preScaling, and the inputs of every row
can tell a wrong kernel from a right one: the oracle's decode -> encode is informative, the given planes differ from it in every
plane of every frame, no map is all zeros or all differences, the three frames of a launch have different words, the 264x70 source
planes hold the boundary and out-of-range codes, and six wrong kernels modelled with the oracle and numpy fail every row they
apply to."""
import numpy as np

from tests.support import frame_kernels as fk
from tests.support import measuring as ms
from tests.support import plane_kernels as pk
from tests.support.host import BLOCKS, SENTINEL, gaps_intact, neither_path_is_vacuous, plane_rows, plane_samples
from tests.support.moments import MOM_BLOCKS, sse_of

ROWS = pk.plane_matrix()
MEASURING = [r for r in ROWS if r.family != "transcode"]
E_KEYS = sorted({(r.scfg, r.dcfg, r.sp, r.dp, r.w, r.h, r.src_sc, r.dst_sc) for r in ROWS})


def test_the_matrix_covers_what_the_docstring_says():
    """per family 48 k_*<CSD, SUBD, CSE, SUBE, VW, LM>: {Lu'v', YCbCr} x SUBD x {(Lu'v', 3), (Lu'v', 7), (YCbCr, 5)} x SUBE x VW {4, 2}"""
    assert len({r.id for r in ROWS}) == len(ROWS)
    kernels = {pk.kernel_of(r) for r in ROWS}
    print("%d rows, %d distinct kernels: %s" % (len(ROWS), len(kernels), ", ".join("%d %s" % (sum(k[0] == f for k in kernels), f) for f in pk.FAMILIES)))
    assert len(kernels) == 192
    full = {(csd, subd, cse, sube, vw, lm) for csd in (fk.LUV, fk.YCC) for subd in (True, False) for (cse, lm) in ((fk.LUV, 3), (fk.LUV, 7), (fk.YCC, 5))
            for sube in (True, False) for vw in (4, 2)}
    assert len(full) == 48
    for family in pk.FAMILIES:
        assert {k[1:] for k in kernels if k[0] == family} == full, family
        blocks = {"transcode": {None}, "distortion": {None}, "distortion_map": set(BLOCKS), "moments_map": set(MOM_BLOCKS)}[family]
        for csd in pk.SOURCES:
            for (cse, lm) in pk.TARGETS:
                rows = [r for r in ROWS if (r.family, r.csd, r.cse, r.lm) == (family, csd, cse, lm)]
                # every block size on the size with several block columns and rows
                assert {r.block for r in rows if (r.w, r.h) == (264, 70)} == blocks, (family, csd, cse, lm)
                if csd == fk.YCC:   # with sc == 1, with the short division and with the complete functions' IEEE division
                    assert {pk.sc_mode(r.src_sc) for r in rows} == {0, 1, 2}, (family, cse, lm)
                    far = [r for r in rows if pk.sc_mode(r.src_sc) == 2]
                    assert [(r.w, r.h, r.sp, r.dp) for r in far] == [(258, 6, 2, 2)], (family, cse, lm)
                else:
                    assert {r.src_sc for r in rows} == {1.0}, (family, cse, lm)
        for k in {k for k in kernels if k[0] == family and k[1] == fk.YCC}:
            modes = {pk.sc_mode(r.src_sc) for r in ROWS if pk.kernel_of(r) == k}
            assert {0, 1} <= modes, (k, modes)
        # the 8-bit profiles: four rows per colour-space pair, the 8-bit table on the side stored in 8 bits
        for (csd, cse) in pk.PAIRS:
            eight = [r for r in ROWS if (r.family, r.csd, r.cse) == (family, csd, cse) and min(r.sp, r.dp) < 2]
            assert [((r.sp, r.dp), (r.w, r.h)) for r in eight] == list(pk.EIGHT_BIT), (family, csd, cse)
            assert all((r.scfg[1] == 8) == (r.sp < 2) and (r.dcfg[1] == 8) == (r.dp < 2) and r.lm == (5 if cse == fk.YCC else 3) for r in eight)
    stats = [r.stats for r in ROWS if r.family == "transcode"]
    assert all(not r.stats for r in MEASURING) and 0.4 < sum(stats) / len(stats) < 0.6
    assert {(r.w, r.h) for r in ROWS if r.stats} == set(pk.SIZES) and {pk.kernel_of(r)[1:5] for r in ROWS if r.stats} == {k[:4] for k in full}


def test_the_source_planes_hold_the_planted_codes():
    """in range everywhere else, three different frames, and 0, 1, the largest code, the one behind it and all ones in the corner of
    264x70: a chroma code beyond the largest in every 16-bit source"""
    for (cfg, profile, w, h) in sorted({(r.scfg, r.sp, r.w, r.h) for r in ROWS}):
        s = pk.source_planes(cfg, profile, w, h)
        assert len(s) == pk.NF
        for p in range(3):
            top = (1 << (cfg[1] if p == 0 else cfg[3])) - 1
            v = [pk.plane_values(s[f][p], profile) for f in range(pk.NF)]
            assert not np.array_equal(v[0], v[1]) and not np.array_equal(v[1], v[2]) and not np.array_equal(v[0], v[2])
            for f in range(pk.NF):
                assert v[f].shape == (plane_rows(w, h, profile, p)[0], (w // 2 if (p and profile in (0, 2)) else w))
                if (w, h) == (264, 70):
                    sub = 2 if (p and profile in (0, 2)) else 1
                    corner = v[f][:8 // sub, :16 // sub]
                    want = {0, 1, top, top + 1, 0xFFFF} if profile > 1 else {0, 1, 0xFF}
                    assert set(np.unique(corner)) == want, (cfg, profile, p, f)
                    assert profile < 2 or (corner > top).any(), (cfg, profile, p, f)
                    v[f][:8 // sub, :16 // sub] = 0
                assert v[f].min() >= 0 and v[f].max() <= top, (cfg, profile, w, h, p, f)


def test_the_oracles_planes_are_informative(oracle_mod):
    """at least 64 distinct sample values in every plane the oracle's decode -> encode makes of a row's source planes at 264x70 and
    258x6, U and V different"""
    least = {}
    for k in E_KEYS:
        (w, h), dp = k[4:6], k[3]
        if (w, h) != (6, 4):
            n = fk.informative(pk.expected(oracle_mod, *k).e, w, h, dp, k)
            least[(w, h)] = min(n, least.get((w, h), n))
    print("%d reference launches; the fewest distinct sample values of an expected plane: %s" %
          (len(E_KEYS), ", ".join("%d at %dx%d" % (n, w, h) for (w, h), n in sorted(least.items()))))
    assert min(least.values()) >= fk.MIN_DISTINCT


def test_every_measuring_row_can_tell_a_wrong_kernel(oracle_mod):
    """the conditions on the given planes, asserted on the reference alone"""
    least = None
    for r in MEASURING:
        gv = pk.given_of(oracle_mod, r)
        nd = gv.dist[:, :, 3]
        assert (nd > 0).all(), (r.id, "a plane of a frame without a difference", nd)
        least = int(nd.min()) if least is None else min(least, int(nd.min()))
        for a in range(pk.NF):
            for b in range(a + 1, pk.NF):
                assert not np.array_equal(gv.words[a], gv.words[b]), (r.id, a, b, "two frames with the same words")
        if r.family != "distortion":
            neither_path_is_vacuous(gv.dmap, (r.id,))
            nby, nbx = -(-r.h // r.block), -(-r.w // r.block)
            assert gv.words.shape == (pk.NF, nby, nbx, 3, 4 if r.family == "distortion_map" else 5), r.id
        if r.family == "moments_map":   # (the two numpy models agree on what they share)
            assert np.array_equal(sse_of(gv.words), gv.dmap[..., 0]), r.id
    print("%d measuring rows; the smallest n_differ of a plane of a frame: %d" % (len(MEASURING), least))


def layouts_of(w, h, profile):
    out = {"wide": (None, 48, 0), "odd": fk.odd_layout(w, h, profile) + (1,)}
    if (w, h) == (264, 70):
        st, base = ms.half_aligned_layout(w, h, profile)
        out["half"] = (st, 48, base)
    return out


def test_the_layouts_are_what_their_names_say(oracle_mod):
    """odd: every base, row stride and frame stride odd; half: the planes half a four-sample unit off, strides multiples of 8 -- good
    for units of two samples; and the same samples and sentinels come out under every layout"""
    for profile in range(4):
        for (w, h) in pk.SIZES[:2]:
            lay = layouts_of(w, h, profile)
            st, gap, base = lay["odd"]
            hp = ms.HostPlanes([], w, h, profile, st, gap, base=base)
            assert base % 2 == 1 and all(s % 2 == 1 for s in hp.st) and all(x % 2 == 1 for x in hp.pfs)
            if "half" in lay:
                st, gap, base = lay["half"]
                hp = ms.HostPlanes([], w, h, profile, st, gap, base=base)
                unit = 8 if profile > 1 else 4       # four samples
                assert base % unit == unit // 2 and all(s % 8 == 0 for s in hp.st) and all(x % 8 == 0 for x in hp.pfs)
                assert base % (unit // 2) == 0 and all(s % (unit // 2) == 0 for s in hp.st + tuple(hp.pfs))
    seen = set()
    for r in ROWS:
        for planes, profile in ((pk.expected_of(oracle_mod, r).s, r.sp), (pk.expected_of(oracle_mod, r).e, r.dp)):
            if (id(planes), profile) in seen or (r.w, r.h) == (6, 4):
                continue
            seen.add((id(planes), profile))
            for name, (st, gap, base) in layouts_of(r.w, r.h, profile).items():
                hp = ms.HostPlanes(planes, r.w, r.h, profile, st, gap, base)
                assert gaps_intact(hp.bufs, r.w, r.h, profile, pk.NF, hp.st, hp.gap, hp.base) and (hp.bufs[0][:hp.base] == SENTINEL).all(), (r.id, name)
                assert fk.planes_problem(hp.bufs, planes, r.w, r.h, profile, hp.st, hp.gap, hp.base) is None, (r.id, name)
                for f in range(pk.NF):
                    for p in range(3):
                        assert np.array_equal(plane_samples(hp.frame(hp.bufs, f)[p], r.w, r.h, profile, p),
                                              plane_samples(planes[f][p], r.w, r.h, profile, p)), (r.id, name, f, p)


def test_every_row_fails_the_modelled_wrong_kernels(oracle_mod):
    """U and V swapped, two frames swapped, a YCbCr source's `/ sc` dropped, 4:2:0 chroma from the top-left pixel, only the first of
    four replicated chroma codes stored, one sample of the last column off by one (tests/support/plane_kernels.py wrong_kernels):
    the comparison of every row they apply to fails for each, and passes for the oracle's own planes"""
    counts = {}
    for r in ROWS:
        assert not pk.tells(oracle_mod, r, pk.expected_of(oracle_mod, r).e), (r.id, "the expectation itself is told from a right kernel")
        wrong = pk.wrong_kernels(oracle_mod, r)
        want = {"uv_swapped", "frames_swapped_0", "frames_swapped_1", "last_column"}
        want |= {"sc_dropped"} if (r.csd == fk.YCC and r.src_sc != 1.0) else set()
        want |= {"top_left_chroma"} if (r.sp in (1, 3) and r.dp in (0, 2)) else set()
        want |= {"first_of_four"} if (r.sp in (0, 2) and r.dp in (1, 3)) else set()
        assert set(wrong) == want, (r.id, sorted(wrong))
        for name, planes in wrong.items():
            assert pk.tells(oracle_mod, r, planes), (r.id, name, "passes this row")
            counts[name] = counts.get(name, 0) + 1
    print("%d rows; rows that fail each wrong kernel: %s" % (len(ROWS), ", ".join("%s %d" % kv for kv in sorted(counts.items()))))
    assert counts["sc_dropped"] > 0 and counts["top_left_chroma"] > 0 and counts["first_of_four"] > 0
