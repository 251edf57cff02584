"""What tests/test_gpu_decode_kernels.py relies on, checked without a GPU: the decode matrix names the 48 k_decode<CS, SUB, VW, GL = false,
DISP = false, YT, RB, OUT16> instantiations its docstring says, every call form meets every (colour space, variant), both 8-bit
profiles occur on every (colour space, variant, frame type), and the inputs of every row can tell a wrong kernel from a right one:
the oracle's frames are informative, the source planes hold the boundary and out-of-range codes, the comparison of a call's buffers
with the expectation (tests/support/decode_kernels.py frames_problem) rejects each error planted into them, and seven wrong kernels
modelled with the oracle and numpy fail every row they apply to."""
import numpy as np

from tests.support import decode_kernels as dk
from tests.support import frame_kernels as fk
from tests.support.host import SENTINEL, float_to_half_np

ROWS = dk.decode_matrix()


def test_the_matrix_covers_what_the_docstring_says():
    """16 float kernels -- Lu'v', RGB, plain YCbCr and XYZ by 4:2:0 / 4:4:4 by VW 4 / 2 --, four with YT, four with YT and RB, and the
    same 24 with OUT16; every form on every (colour space, variant); profiles 0 and 1 on every (colour space, variant, frame type);
    a YCbCr variant with sc_mode 0, 1 and 2; four frames on the rotating rows"""
    assert len({r.id for r in ROWS}) == len(ROWS)
    kernels = {dk.row_kernel(r) for r in ROWS}
    print("%d rows, %d distinct kernels" % (len(ROWS), len(kernels)))
    assert len(kernels) == 48 and kernels == dk.all_kernels()
    plain = {k for k in kernels if not k[3] and not k[5]}
    assert len(plain) == 16 and {k[0] for k in plain} == {fk.LUV, fk.RGB, fk.YCC, fk.XYZ}
    assert {k for k in kernels if k[3] and not k[4] and not k[5]} == {(fk.YCC, sub, vw, True, False, False) for sub in (True, False) for vw in (4, 2)}
    assert {k for k in kernels if k[4] and not k[5]} == {(fk.YCC, sub, vw, True, True, False) for sub in (True, False) for vw in (4, 2)}
    assert {k[:5] for k in kernels if k[5]} == {k[:5] for k in kernels if not k[5]}
    for (cs, variant) in dk.CASES:
        rows = [r for r in ROWS if (r.cs, r.variant) == (cs, variant)]
        assert {r.form for r in rows if not r.out16} == set(dk.FLOAT_FORMS), (cs, variant)
        assert {r.form for r in rows if r.out16} == set(dk.HALF_FORMS), (cs, variant)
        for vw in (4, 2):   # (and every form meets both vector widths of the pair)
            assert {r.form for r in rows if not r.out16 and dk.row_kernel(r)[2] == vw} == set(dk.FLOAT_FORMS), (cs, variant, vw)
            assert {r.form for r in rows if r.out16 and dk.row_kernel(r)[2] == vw} == set(dk.HALF_FORMS), (cs, variant, vw)
        for out16 in (False, True):
            assert {r.profile for r in rows if r.out16 == out16} == {0, 1, 2, 3}, (cs, variant, out16)
            assert all(r.cfg == fk.pq8(cs) for r in rows if r.profile < 2) and all(r.cfg[1] == (10 if cs == fk.YCC else 11) for r in rows if r.profile > 1)
        assert {dk.sc_mode(r.sc) for r in rows} == ({0, 1, 2} if cs == fk.YCC else {0, 1}), (cs, variant)
        assert all(r.tunes == (dk.VARIANTS[variant] if cs == fk.YCC else ()) for r in rows)
    for k in kernels:   # every kernel with and without a division by its preScaling
        assert {0, 1} <= {dk.sc_mode(r.sc) for r in ROWS if dk.row_kernel(r) == k}, k
    assert {r.sc for r in ROWS} == {1.0, 20.0, dk.SC_FAR} and {(r.w, r.h) for r in ROWS} == set(dk.SIZES)
    assert all(dk.nframes(r.form) == (4 if r.form == "rotating" else 3) for r in ROWS)
    assert all(r.form != "rotating" for r in ROWS if r.out16)


def test_kernel_of_follows_the_alignment_of_the_output():
    """VW 4 needs w % 4 == 0, pointers aligned to four elements and a frame stride % 4 == 0; the tunes decide YT and RB"""
    args = (fk.YCC, 2, 64)
    assert dk.kernel_of(*args, True, 3 * 64 * 32 + 4, (), False) == (fk.YCC, True, 4, True, True, False)
    assert dk.kernel_of(*args, False, 3 * 64 * 32 + 4, (), False)[2] == 2
    assert dk.kernel_of(*args, True, 3 * 64 * 32 + 2, (), True)[2] == 2
    assert dk.kernel_of(fk.YCC, 3, 258, True, 3 * 258 * 6 + 4, (), False)[1:3] == (False, 2)
    assert dk.kernel_of(*args, True, 4, dk.VARIANTS["plain"], False)[3:5] == (False, False)
    assert dk.kernel_of(*args, True, 4, dk.VARIANTS["yt"], False)[3:5] == (True, False)
    assert dk.kernel_of(*args, True, 4, dk.VARIANTS["rb"] + (("block", 64),), True)[3:] == (True, True, True)
    assert dk.kernel_of(fk.LUV, 2, 64, True, 4, dk.VARIANTS["rb"], False)[3:5] == (False, False)
    for form in dk.FLOAT_FORMS:
        lay = dk.OutLayout(form, dk.nframes(form), 64, 32, False)
        assert lay.aligned4 and lay.fs % 4 == 0
        assert not dk.OutLayout(form, dk.nframes(form), 64, 32, False, base=2).aligned4
    rot = dk.OutLayout("rotating", 4, 6, 4, False)
    assert [rot.at(f, 0)[0] for f in range(4)] == [0, 1, 2, 0] and rot.at(3, 0)[1] == rot.base + rot.fs
    assert rot.elements == [rot.base + 2 * rot.fs, rot.base + rot.fs, rot.base + rot.fs]


def test_the_source_planes_hold_the_planted_codes():
    """in range everywhere else, distinct frames, and in the corner of 264x70 and of 258x6 the codes 0, 1, maxVal - 1, maxVal,
    maxVal + 1, maxC, maxC + 1 and all ones that the sample holds: a chroma code beyond maxC in every 16-bit Lu'v' and YCbCr row of
    those sizes, and in no 8-bit row (the 8-bit tables' maxC is all ones or beyond the sample)"""
    seen = 0
    for r in ROWS:
        s = dk.source_planes(r.cfg, r.profile, r.w, r.h, dk.nframes(r.form), dk.is_picture(r))
        ones = 0xFFFF if r.profile > 1 else 0xFF
        codes = set(dk.planted_codes(r.cfg, r.profile))
        for p in range(3):
            top = min((1 << (r.cfg[1] if p == 0 else r.cfg[3])) - 1, ones)
            v = [dk.plane_values(fr[p], r.profile).copy() for fr in s]
            for f in range(len(s)):
                for g in range(f + 1, len(s)):
                    assert not np.array_equal(v[f], v[g]), (r.id, p, f, g)
                if (r.w, r.h) in dk.PLANTED_ROWS:
                    sub = 2 if (p and r.profile in (0, 2)) else 1
                    cr, cc = dk.PLANTED_ROWS[(r.w, r.h)] // sub, dk.PLANTED_COLUMNS // sub
                    assert set(np.unique(v[f][:cr, :cc])) == codes, (r.id, p, f)
                    v[f][:cr, :cc] = 0
                assert v[f].min() >= 0 and v[f].max() <= top, (r.id, p, f)
        want = r.cs in (fk.LUV, fk.YCC) and r.profile > 1 and (r.w, r.h) in dk.PLANTED_ROWS
        assert dk.chroma_out_of_range(r, s) == want, r.id
        seen += want
    assert seen > 0
    # the picture-like frames are smooth: neighbouring luma codes a few codes apart, unlike the unrelated frame between them
    r = next(r for r in ROWS if dk.is_picture(r) and r.profile == 2)
    s = dk.source_planes(r.cfg, r.profile, r.w, r.h, 3, True)
    step = [np.abs(np.diff(dk.plane_values(fr[0], r.profile)[16:], axis=1)).mean() for fr in s]
    assert step[0] < 16 and step[2] < 16 and step[1] > 200, step


def test_the_expected_frames_are_informative(oracle_mod):
    """at least 64 distinct finite values in every channel of every expected frame (6x4 exempt), the channels of a frame different, the
    frames of a launch different; the smallest count is printed"""
    least = {}
    for r in ROWS:
        n = dk.informative(dk.expected(oracle_mod, r).want, (r.id,))
        if (r.w, r.h) != (6, 4):
            key = "f16" if r.out16 else "f32"
            least[key] = min(n, least.get(key, n))
    print("%d rows; the fewest distinct finite values of an expected channel: %s" % (len(ROWS), ", ".join("%d %s" % (n, k) for k, n in sorted(least.items()))))
    assert min(least.values()) >= dk.MIN_DISTINCT


def test_the_comparison_rejects_each_planted_error(oracle_mod):
    """one float one ulp off in the last row and column of the last frame, a half one code off there, a NaN for a number, a changed
    sentinel byte behind a frame, behind the last frame, in front of the first -- in every form"""
    for r in [next(r for r in ROWS if (r.form, r.out16, r.w) == (form, out16, 258)) for out16 in (False, True)
              for form in (dk.HALF_FORMS if out16 else dk.FLOAT_FORMS)]:
        want = dk.expected(oracle_mod, r).want
        lay = dk.layout_of(r)
        good = lay.filled(want)
        assert dk.frames_problem(dk.Written(lay, good), want) is None, r.id
        assert all((b == SENTINEL).all() for b in lay.blank())
        f, h, w = lay.nf - 1, lay.h, lay.w

        def planted(change):
            bufs = [b.copy() for b in good]
            change(bufs)
            return dk.frames_problem(dk.Written(lay, bufs), want)

        for c in range(3):
            b, off = lay.at(f, c)
            last = off + lay.n - 1

            def one_off(bufs, b=b, last=last):
                bufs[b].view(np.uint16 if r.out16 else np.uint32)[last] ^= 1
            text = planted(one_off)
            assert text is not None and text.startswith("frame %d channel %d row %d column %d:" % (f, c, h - 1, w - 1)), (r.id, text)
            assert "expected" in text and "1 of %d" % lay.n in text, text

            def nan(bufs, b=b, last=last):
                bufs[b].view(np.uint16 if r.out16 else np.uint32)[last] = 0x7E00 if r.out16 else 0x7FC00000
            assert planted(nan) is not None, (r.id, c)
        esz = lay.dtype.itemsize
        b, off = lay.at(0, 2)
        places = {"the first byte behind a frame": (b, (off + lay.n) * esz), "the last byte of the gap behind it": (b, (off + lay.n + lay.pad) * esz - 1),
                  "the last byte of the buffer": (b, good[b].size - 1), "the first byte of the buffer": (b, 0),
                  "the last byte in front of the first frame": (lay.at(0, 0)[0], lay.base * esz - 1)}
        for what, (b, at) in places.items():
            def stray(bufs, b=b, at=at):
                assert bufs[b][at] == SENTINEL, (what, "is no byte outside the frames")
                bufs[b][at] ^= 0x10
            text = planted(stray)
            assert text is not None and "buffer %d: byte %d outside the frames" % (b, at) in text, (r.id, what, text)
    # two NaN with different payloads are the same; a NaN and a number are not
    lay = dk.OutLayout("packed", 3, 6, 4, False)
    fr = np.arange(3 * 3 * 24, dtype=np.float32).reshape(3, 3, 4, 6)
    fr[1, 1, 2, 3] = np.nan
    other = fr.copy()
    other.view(np.uint32)[1, 1, 2, 3] = 0x7FC00001
    assert dk.frames_problem(dk.Written(lay, lay.filled(other)), fr) is None
    other[1, 1, 2, 3] = 0.0
    assert "frame 1 channel 1 row 2 column 3" in dk.frames_problem(dk.Written(lay, lay.filled(other)), fr)


def test_truncation_differs_from_rounding_where_it_should():
    x = np.array([1.0, 1.0 + 2.0 ** -11, 1.0 + 2.0 ** -10 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -12, -1.0 - 3 * 2.0 ** -12, 65519.0, 7e4, np.inf, 3e-8, 0.0],
                 dtype=np.float32)
    r, t = float_to_half_np(x), dk.truncated(x)
    assert r.tolist() == [0x3C00, 0x3C00, 0x3C02, 0x3C01, 0xBC01, 0x7BFF, 0x7C00, 0x7C00, 0x0001, 0x0000]
    assert t.tolist() == [0x3C00, 0x3C00, 0x3C01, 0x3C00, 0xBC00, 0x7BFF, 0x7BFF, 0x7C00, 0x0000, 0x0000]


def test_every_row_fails_the_modelled_wrong_kernels(oracle_mod):
    """U and V swapped, two frames swapped, a dropped `/ sc`, 4:2:0 chroma from the neighbouring quad, an out-of-range chroma code
    clamped, the last column's luma code off by one, binary16 by truncation (tests/support/decode_kernels.py wrong_kernels): the
    comparison of every row a fault applies to fails for it and passes for the oracle's own frames; which rows cannot tell a fault
    apart is printed with the reason; every kernel that has the faulty code has a row that tells"""
    told, cannot = {}, {}
    for r in ROWS:
        ex = dk.expected(oracle_mod, r)
        assert not dk.tells(oracle_mod, r, ex.want), (r.id, "the expectation itself is told from a right kernel")
        wrong = dk.wrong_kernels(oracle_mod, r)
        want = {"uv_swapped", "frames_swapped", "last_column"}
        for name, here, why in (("sc_dropped", r.sc != 1.0, "the rows with preScaling 1: there is no division to drop"),
                                ("neighbour_quad", r.profile in (0, 2), "the rows of profiles 1 and 3: every pixel has its own chroma sample"),
                                ("chroma_clamped", dk.chroma_out_of_range(r, ex.s),
                                 "the rows whose planes hold no chroma code beyond maxC that a complete function would take: RGB and XYZ (every "
                                 "plane goes through the table read, which clamps), profiles 0 and 1 (maxC is all ones or more), 64x32 and 6x4 "
                                 "(no planted corner)"),
                                ("truncated", r.out16, "the rows with float frames: nothing is narrowed")):
            if here:
                want.add(name)
            else:
                cannot.setdefault((name, why), []).append(r.id)
        assert set(wrong) == want, (r.id, sorted(wrong))
        for name, frames in wrong.items():
            assert dk.tells(oracle_mod, r, frames), (r.id, name, "passes this row")
            told.setdefault(name, set()).add(dk.row_kernel(r))
    for (name, why), ids in sorted(cannot.items()):
        print("%s: %d of %d rows cannot tell it apart -- %s" % (name, len(ids), len(ROWS), why))
    for name, kernels in sorted(told.items()):
        missing = {k for k in dk.all_kernels() if dk.applies(name, k)} - kernels
        print("%s: told apart on rows of %d kernels" % (name, len(kernels)))
        assert not missing, (name, "no row of these kernels tells it apart", sorted(missing))
    assert set(told) == {"uv_swapped", "frames_swapped", "sc_dropped", "neighbour_quad", "chroma_clamped", "last_column", "truncated"}
