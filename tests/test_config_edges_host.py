"""What tests/test_gpu_config_edges.py relies on, checked without a GPU: the record counts and byte sums of tests/support/config_edges.py
recomputed with the library's host code (lumahip_build_lut, lumahip_thresh_index_host, lumahip_lin_index_host,
lumahip_ycbcr_luma_index_host), which rows are accepted and which refused -- derived from those sums and the budget --, that the rows
reach every family, that the inputs reach both ends of every staged table, that the oracle's expectation of every accepted row is
informative, and that five wrong kernels modelled with the oracle and numpy fail every row they apply to."""
import numpy as np

from lumahdrv_amd import capi
from tests.support import config_edges as ce
from tests.support import plane_kernels as pk
from tests.support.host import neither_path_is_vacuous

FRAME_ROWS, PLANE_ROWS = ce.frame_rows(), ce.plane_rows_all()
KIB = 1024


def lut(cfg):
    return capi.build_lut(cfg[0], cfg[1], cfg[4], cfg[5])


def test_the_record_counts_are_the_librarys():
    """every count the byte sums are made of, from the host code that builds the device's records"""
    for (kind, ptf, bits, max_lum), n in sorted(ce.RECORDS.items()):
        t = capi.build_lut(ptf, bits, max_lum, 0.01 if max_lum == 1000.0 else 0.005)
        assert t.size == 1 << bits
        ix = {"thresh": capi.thresh_index, "lin": capi.lin_index, "composite": lambda m: capi.ycbcr_luma_index(m, max_lum)}[kind](t)
        assert ix["ok"] and ix["nbuckets"] == n, (kind, ptf, bits, max_lum, ix["nbuckets"], n)
        if kind == "lin":
            assert ix["rec"].shape == (n, 2)
    # the counts and rounded bytes the layouts were planned with
    table = {("thresh", ce.PQ, 13, 1e4): (34946, 139792), ("thresh", ce.PQ, 12, 1e4): (16531, 66128), ("thresh", ce.LOG, 12, 1e4): (10722, 42896),
             ("thresh", ce.PQ, 11, 1e4): (7834, None), ("thresh", ce.PQ, 9, 1000.0): (1744, None), ("composite", ce.PQ, 12, 1000.0): (16346, 65392),
             ("composite", ce.PQ, 11, 1000.0): (8177, 32720), ("composite", ce.PQ, 9, 1000.0): (2039, None), ("lin", ce.LINEAR, 13, 1e4): (8209, 65680),
             ("lin", ce.LINEAR, 14, 1e4): (16418, 131344)}
    for key, (n, b) in table.items():
        assert ce.RECORDS[key] == n and (b is None or ce.round16(n * (8 if key[0] == "lin" else 4)) == b), key


def test_the_byte_sums():
    """the sums of the support module's docstring, from its restatement of the host code"""
    assert ce.POWF_WIDE == 39168 and ce.BUDGET == 163840 and ce.HALF_BYTES == 126992
    assert (ce.MEET["distortion"], ce.MEET["distortion_map"], ce.MEET["moments_map"]) == (128, 1536, 3840)
    # S1
    assert ce.search(ce.S1) == (3, 139792, 0) and ce.encode_lds(ce.S1) == 139792 and ce.decode_lds(ce.S1) == 32784 + 16384
    assert ce.measuring_lm(ce.S1, False, "moments_map") == (3, 139792) and 139792 + 3840 == 143632 <= ce.BUDGET
    # S2: the largest decode-side layout upload_decode_tables accepts
    assert ce.search(ce.S2) == (3, ce.round16(16592 * 4), 65392) and ce.encode_lds(ce.S2, True) == 104560
    assert ce.has_ytab(ce.S2) and ce.decode_lds(ce.S2) == 39168 + 2 * 16400 + 2 * 16384 == 104736
    assert not ce.half_table_fits(ce.S2)
    # S3: the float-bit records do not fit, the value-keyed ones do
    assert ce.search(ce.S3) == (7, 131344, 0) and ce.decode_lds(ce.S3) == 65552 + 2048
    # S4, S5: sizes that are no multiples of 16 before the padding
    assert ce.search(ce.S4) == (3, 1744 * 4, ce.round16(2039 * 4)) and 2039 * 4 % 16 != 0 and ce.half_table_fits(ce.S4)
    assert ce.search(ce.S5) == (3, ce.round16(177 * 4), 0) and 177 * 4 % 16 != 0 and ce.col_bytes(ce.S5) == 128 and ce.lut_bytes(ce.S5) == 272
    # S6: the table leaves LDS on the decode side only
    assert not ce.lut_in_lds(ce.S6) and ce.decode_lds(ce.S6) == 0 and ce.search(ce.S6)[0] == 3 and not ce.light_accepted(ce.S6)
    # S7: the half-input table fits the encode and the distortion launches, and not beside the moments map
    assert ce.half_table_fits(ce.S7) and ce.encode_lds(ce.S7, True, True) == 32720 + 126992 + 512 == 160224
    assert ce.measuring_lm(ce.S7, True, "distortion") == (6, 160224) and ce.measuring_lm(ce.S7, True, "distortion_map") == (6, 160224)
    assert 160224 + 3840 > ce.BUDGET and ce.measuring_lm(ce.S7, True, "moments_map") == (3, ce.round16(7848 * 4) + 39168)
    # S8: the largest decode-side layout; the records leave LDS, and the measuring calls with them
    assert ce.has_ytab(ce.S8) and ce.decode_lds(ce.S8) == 39168 + 2 * 32784 + 2 * 16384 == 137504 and ce.search(ce.S8) == (4, 0, 0)
    assert 35022 * 4 <= ce.TABLE_MAX and 35022 * 4 + 16 + 39168 > ce.BUDGET and ce.encode_lds(ce.S8) == 39168
    assert not ce.has_ytab((ce.PQ, 14, ce.YCC, 12, 1000.0, 0.01)) and not ce.has_ytab((ce.PQ, 13, ce.YCC, 13, 1000.0, 0.01))
    for sid, cfg in ce.SINGLES.items():     # ... and nowhere else
        for family in ("distortion", "distortion_map", "moments_map"):
            if sid == "S8":
                assert ce.measuring_lm(cfg, False, family) is None and ce.measuring_lm(cfg, True, family) is None
                continue
            want = 6 if ce.half_table_fits(cfg) and (sid, family) != ("S7", "moments_map") else ce.search(cfg)[0]
            assert ce.measuring_lm(cfg, True, family)[0] == want, (sid, family)
            assert ce.measuring_lm(cfg, False, family)[0] == (5 if ce.search(cfg)[2] else ce.search(cfg)[0]), (sid, family)
    sums = {"P1": 16400 + 1024 + 139792, "P2": 16400 + 4096 + 139792, "P3": 16400 + 16384 + 139792, "P3b": 16400 + 8192 + 139792,
            "P4": 39168 + 32800 + 32768 + 42896, "P5": 39168 + 32800 + 32768 + 66128, "P6": 39168 + 17424 + 65392, "P7a": 17424 + 131344,
            "P7b": 55584 + 65680}
    assert (sums["P1"], sums["P2"], sums["P3"], sums["P4"], sums["P5"], sums["P6"], sums["P7a"], sums["P7b"]) == \
        (157216, 160288, 172576, 147632, 170864, 121984, 148768, 121264)
    for pid, b in sums.items():
        assert ce.pair_lds(*ce.PAIRS[pid]) == b, (pid, ce.pair_lds(*ce.PAIRS[pid]), b)
    assert ce.pair_lds(*ce.PAIRS["P8"]) < 64 * KIB


def test_accepted_and_refused_follow_from_the_sums():
    """per family one accepted pair within 4 KiB below the budget and one refused pair within 4 KiB above it; S6 is refused as a source
    by every plane-fed call; the rows reach every family"""
    for family in ce.PLANE_FAMILIES:
        acc = {pid: ce.pair_lds(s, d) + ce.MEET[family] for pid, (s, d) in ce.PAIRS.items() if ce.pair_accepted(family, s, d)}
        ref = {pid: ce.pair_lds(s, d) + ce.MEET[family] for pid, (s, d) in ce.PAIRS.items() if not ce.pair_accepted(family, s, d) and ce.source_taken(s)}
        print(family, "accepted", sorted(acc.items()), "refused", sorted(ref.items()))
        assert ce.BUDGET - 4 * KIB <= max(acc.values()) <= ce.BUDGET and ce.BUDGET < min(ref.values()) <= ce.BUDGET + 4 * KIB, family
        want = {"P1", "P2", "P4", "P6", "P7a", "P7b", "P8"} - ({"P2"} if family == "moments_map" else set())
        assert set(acc) == want and set(ref) == set(ce.PAIRS) - want - {"P9"}, (family, sorted(acc), sorted(ref))
        assert not ce.source_taken(ce.S6) and not ce.pair_accepted(family, *ce.PAIRS["P9"])
    assert {(r.pid, r.family) for r in PLANE_ROWS} == {(p, f) for p in ce.PAIRS for f in ce.PLANE_FAMILIES}
    for pid in ce.PAIRS:
        for family in ce.PLANE_FAMILIES:
            rows = [r for r in PLANE_ROWS if (r.pid, r.family) == (pid, family)]
            assert {(r.sp, r.dp) for r in rows} == set(ce.PROFILE_PAIRS), (pid, family)
            assert {(r.w, r.h) for r in rows} == set(ce.HALF_SIZES if family == "half" else ce.PLANE_SIZES), (pid, family)
            assert {r.src_sc for r in rows} == ({1.0, 20.0} if ce.PAIRS[pid][0][2] == ce.YCC else {1.0}), (pid, family)
    assert {(r.sid, r.call) for r in FRAME_ROWS} == {(s, c) for s in ce.SINGLES for c in ce.FRAME_CALLS}
    for sid in ce.SINGLES:
        rows = [r for r in FRAME_ROWS if r.sid == sid]
        assert {r.profile for r in rows} == ({0, 1} if sid == "S5" else {2, 3}) and {(r.w, r.h) for r in rows} == set(ce.FRAME_SIZES), sid
    assert len({r.id for r in FRAME_ROWS + PLANE_ROWS}) == len(FRAME_ROWS) + len(PLANE_ROWS)
    # the light level of planes: what the decode call stages, depths up to 12
    assert {sid for sid, cfg in ce.SINGLES.items() if ce.light_accepted(cfg)} == {"S2", "S4", "S5", "S7"}
    # the launch shapes run again on the rows whose tables exceed 53 KiB
    bigs = {r.sid if isinstance(r, ce.FrameRow) else r.pid for r in FRAME_ROWS + PLANE_ROWS if ce.big(r)}
    assert bigs == {"S1", "S2", "S3", "S7", "S8","P1", "P2", "P4", "P6", "P7a", "P7b", "P8"}, sorted(bigs)     # (P8: the powf tables alone are 38 KiB)
    for family in ("distortion", "distortion_map", "moments_map"):     # S1 .. S7 come to a mode the measuring calls take, S8 does not
        assert {sid for sid, cfg in ce.SINGLES.items() if all(ce.measuring_lm(cfg, in16, family) is None for in16 in (False, True))} == {"S8"}
        assert all(ce.measuring_lm(cfg, in16, family) is not None for sid, cfg in ce.SINGLES.items() for in16 in (False, True) if sid != "S8")
    for sc in (1.0, 20.0):      # the half-input table exists for both preScalings of the YCbCr rows
        assert capi.ycbcr_half_table(sc, 1000.0) is not None


def test_the_inputs_reach_the_ends_of_every_table(oracle_mod):
    """source planes: codes 0 .. 3 and top - 3 .. top of every plane in every frame, three distinct frames, at 264x70 the out-of-range codes
    too; frames: pixels above the table's largest value and below its smallest positive one"""
    keys = {(r.cfg, r.profile, r.w, r.h) for r in FRAME_ROWS} | {(r.scfg, r.sp, r.w, r.h) for r in PLANE_ROWS if ce.row_accepted(r)}
    for (cfg, profile, w, h) in sorted(keys):
        s = ce.source_planes(cfg, profile, w, h)
        for p in range(3):
            v = [pk.plane_values(s[f][p], profile) for f in range(ce.NF)]
            assert not np.array_equal(v[0], v[1]) and not np.array_equal(v[1], v[2]) and not np.array_equal(v[0], v[2])
            top = (1 << (cfg[1] if p == 0 else cfg[3])) - 1
            for f in range(ce.NF):
                assert set(ce.edge_codes(cfg, p)) <= set(np.unique(v[f])), (cfg, profile, w, h, p, f)
                if (w, h) == (264, 70):
                    assert (v[f] > top).any() or top == 0xFFFF, (cfg, profile, p, f)
                else:
                    assert v[f].max() <= top
    for r in FRAME_ROWS:
        if r.call in ("decode", "light"):
            continue
        t = lut(r.cfg)
        for halves in (False, True):
            fr = np.asarray(ce.frames(oracle_mod, r.cfg, r.w, r.h, r.sc, halves), dtype=np.float32)
            for f in range(ce.NF):
                grey = fr[f, :, r.h - 1, 8 * f:8 * f + 8]
                assert (grey[:, :4] * np.float32(r.sc) > t[-1]).all() and (grey[:, 4:] * np.float32(r.sc) < t[t > 0][0]).all(), (r.id, halves, f)


def test_the_oracles_expectations_are_informative(oracle_mod):
    """asserted on the oracle's planes of every accepted row: the luma plane holds the table's lowest and largest code and at least 64
    distinct values (S5: every code), U differs from V, the frames differ pairwise; the measuring rows: every given plane of every frame
    differs from the expectation, no map is all zeros or all differences, the frames' words differ pairwise"""
    for r in FRAME_ROWS:
        if r.call in ("decode", "light"):
            d = ce.frame_expected(oracle_mod, r.cfg, r.profile, r.w, r.h, r.sc).d
            assert all(not np.array_equal(d[a].view(np.uint32), d[b].view(np.uint32)) for a in range(ce.NF) for b in range(a + 1, ce.NF)), r.id
            continue
        for halves in (False, True):
            ce.luma_informative(oracle_mod, ce.frame_expected(oracle_mod, r.cfg, r.profile, r.w, r.h, r.sc, halves).e, r.w, r.h, r.profile, r.cfg, r.sc, (r.id, halves))
    low = ce.black_code(oracle_mod, ce.S5, 1.0)
    print("S5: an encode produces the luma codes %d .. 63" % low)
    for fr in ce.frame_expected(oracle_mod, ce.S5, 0, 64, 32, 1.0).e:
        assert set(np.unique(np.asarray(fr[0])[:, :64])) == set(range(low, 64))
    for r in PLANE_ROWS:
        if ce.row_accepted(r):
            ce.plane_row_informative(oracle_mod, r)
    for r in FRAME_ROWS + PLANE_ROWS:
        family = r.call if isinstance(r, ce.FrameRow) else r.family
        if family not in ce.BLOCKS or not ce.row_accepted(r):
            continue
        for block in ce.BLOCKS[family]:
            for halves in ((False, True) if isinstance(r, ce.FrameRow) else (False,)):
                g, words, dist, dmap = ce.given(oracle_mod, r, block, halves)
                assert (dist[:, :, 3] > 0).all(), (r.id, block, "a plane of a frame without a difference")
                assert all(not np.array_equal(words[a], words[b]) for a in range(ce.NF) for b in range(a + 1, ce.NF)), (r.id, block)
                if family != "distortion":
                    neither_path_is_vacuous(dmap, (r.id, block))


def test_every_row_fails_the_modelled_wrong_kernels(oracle_mod):
    """the end of the luminance table zeroed, the end of the colour table(s) zeroed, the colour table read 16 bytes too far, the y table and
    the luminance table exchanged, the top of the records lost (tests/support/config_edges.py wrong_decodes, records_top_lost): the
    comparison of every accepted row they apply to fails for each, and passes for the oracle's own result"""
    counts = {}
    for r in FRAME_ROWS + PLANE_ROWS:
        if not ce.row_accepted(r):
            continue
        family = r.call if isinstance(r, ce.FrameRow) else r.family
        for halves in ((False, True) if isinstance(r, ce.FrameRow) else (False,)):
            if family == "light" and halves:
                continue
            wrong = ce.wrong_results(oracle_mod, r, halves)
            assert set(wrong) == ce.expected_names(r), (r.id, sorted(wrong))
            ex = ce.plane_expected(oracle_mod, r) if isinstance(r, ce.PlaneRow) else ce.frame_expected(oracle_mod, r.cfg, r.profile, r.w, r.h, r.sc, halves)
            right = ex.d if family == "decode" else ce.ll.model_frames(ex.d, 1.0) if family == "light" else ex.e
            for block in ce.BLOCKS.get(family, (None,)):
                assert not ce.tells(oracle_mod, r, right, block, halves), (r.id, block, halves, "the expectation itself is told from a right kernel")
                for name, result in wrong.items():
                    assert ce.tells(oracle_mod, r, result, block, halves), (r.id, block, halves, name, "passes this row")
                    counts[name] = counts.get(name, 0) + 1
    print("rows (by block and frame type) that fail each wrong kernel: %s" % ", ".join("%s %d" % kv for kv in sorted(counts.items())))
    assert set(counts) == set(ce.WRONG)
