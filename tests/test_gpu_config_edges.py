"""The LDS-staging kernels at the edges of the quantizer space -- needs an MI355X.

The layout of the staged tables is stated twice, in the kernels (luma_kernels.hpp stage_tables, lds_quant_bytes) and in the host code that
sizes the dynamic LDS, accepts or refuses a configuration against the 160 KiB of a workgroup and picks the workgroup size
(lumahip_launch.hip lds_bytes, lumahip_transcode.hip transcode_plan, lumahip_core.hip upload_decode_tables / records_fit_lds,
lumahip_distortion.hip distortion_plan, lumahip_light_level.hip).  A disagreement does not fault: an LDS access past the allocation
reads zero or is dropped, and the highest codes of whichever table comes last come out wrong.  tests/support/config_edges.py lists the
configurations (S1 .. S8, P1 .. P9) whose sizes expose one, restates the host's sums, and makes inputs that reach both ends of every table;
tests/test_config_edges_host.py holds those sums to the library's host code and the inputs to the conditions that let a row fail.

Every comparison of planes, frames and words is exact equality with the ORACLE (decode; encode; decode -> [2x2 box ->] encode) or numpy
(the measuring words, the light-level model); the one tolerance is the statistics' sum (fk.stats_problem, 1e-4).  Destinations hold the
sentinel in the wide layout, output words the 0xC3 pattern with 16 guard words behind them, and every input is byte for byte what it
was.  Every accepted row asserts the front end first: the search mode, for YCbCr whether the half-input table exists, and
quantizer_info's LDS bytes against the support module's own count.
  test_frame_rows   S1 .. S8 x {encode, decode (both also with binary16 frames), the three frame-fed measuring calls (float and binary16
                    frames), the light level of planes} x two profiles x 64x32 (VW 4) and 258x6 (VW 2, ragged); statistics on every other
                    encode row; map blocks 16 and 64, moments blocks 8 and 64.  lumahip_half_table_info's "table_launches" says which
                    encode kernel ran (the measuring calls do not count theirs: that S7's binary16 moments map falls back to the
                    search of the mode is derived from the sums, not observed).  S8's search mode (4) is refused by the measuring calls,
                    S1, S3, S6 and S8 by the light level of planes
  test_plane_rows   P1 .. P9 x {k_transcode, its three measuring siblings, k_transcode_half} x profile pairs (2, 2) (3, 2) (2, 3) x two
                    sizes, a YCbCr source with both preScalings
Rows whose tables exceed 53 KiB run again under "block" 1024 and under "grid_enc" 2, "block" 64: the planes, frames and words of the
default launch.  A refused row asserts LUMAHIP_ERR_UNSUPPORTED, a non-empty lumahip_last_error and an untouched destination or output;
the same context then completes an accepted call."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.support import config_edges as ce  # noqa: E402
from tests.support import frame_kernels as fk  # noqa: E402
from tests.support import light_level as ll  # noqa: E402
from tests.support import measuring as ms  # noqa: E402
from tests.support import plane_kernels as pk  # noqa: E402
from tests.support.decode_kernels import differ  # noqa: E402
from tests.support.device import (FloatOut, Frames, L, Planes, ctx, dist, dist_map, encode, measure, on_device, stats_buf, tmap,  # noqa: E402,F401
                                  transcoded)
from tests.support.host import ERR_UNSUPPORTED, GUARD, OUT_FILL, widen_halves  # noqa: E402
from tests.support.moments import mom_map  # noqa: E402
from tests.support.transcode_moments import tmom  # noqa: E402

NF = ce.NF
FRAME_ROWS, PLANE_ROWS = ce.frame_rows(), ce.plane_rows_all()
_ctx = {}


def context(L, cfg, scfg=None, tunes=()):
    """a context on torch's stream per (configuration, source configuration, tunes), made once"""
    key = (cfg, scfg, tuple(tunes))
    if key not in _ctx:
        c = ctx(L, cfg, scfg)
        for name, v in tunes:
            c.tune(name, v)
        _ctx[key] = c
    return _ctx[key]


def shapes_of(row):
    """the default launch and, for tables beyond 53 KiB, the two other launch shapes"""
    return [("default", ())] + (list(ce.SHAPES.items()) if ce.big(row) else [])


def front_end_asserted(c, cfg, sc, tag):
    info = c.quantizer_info()
    assert info["mode"] == ce.search(cfg)[0], tag + (info,)
    assert info["lds_bytes"] == ce.encode_lds(cfg), tag + (info, ce.encode_lds(cfg))
    if cfg[2] == ce.YCC:
        half = c.half_table_info(sc)
        assert half["used"] == ce.half_table_fits(cfg), tag + (half,)
        assert half["lds_bytes"] == (ce.encode_lds(cfg, True, True) if half["used"] else 0), tag + (half,)


def refused(L, c, call, untouched, tag):
    import torch
    with pytest.raises(L.LumaHipError) as e:
        call()
    assert e.value.code == ERR_UNSUPPORTED, tag + (str(e.value),)
    assert c.L.lumahip_last_error(c.h).decode() != "", tag
    torch.cuda.synchronize()
    assert untouched(), tag + ("a refused call wrote to its destination",)


def laid_out(L, frames, w, h, profile):
    return on_device(L, ms.HostPlanes(frames, w, h, profile))


def words_buf(n):
    import torch
    from tests.support.device import dev
    return torch.full((n + GUARD,), OUT_FILL, dtype=torch.int64, device=dev())


# ---- 1. one quantizer
def alternate(profile, size, sizes):
    """every other row of a (configuration, call): each profile and each size meets both"""
    return (profile % 2 + sizes.index(size)) % 2 == 0


def encode_row(L, o, c, row):
    import torch
    stats = alternate(row.profile, (row.w, row.h), ce.FRAME_SIZES)
    default = None
    for shape, tunes in shapes_of(row):
        cs = context(L, row.cfg, None, tunes)
        front_end_asserted(cs, row.cfg, row.sc, (row.id, shape))
        for halves in (False, True):
            ex = ce.frame_expected(o, row.cfg, row.profile, row.w, row.h, row.sc, halves)
            fr = Frames(ex.frames, dtype=np.float16 if halves else np.float32)
            pl = Planes(L, row.w, row.h, row.profile, NF, strides=fk.wide_layout(row.w, row.h, row.profile))
            sd = stats_buf(NF) if stats else None
            before = cs.half_table_info(row.sc)["table_launches"]
            (cs.encode_frames_device_f16 if halves else cs.encode_frames_device)(fr.ptr, fr.fs, NF, row.w, row.h, row.sc, row.profile, pl.ptrs, pl.st,
                                                                                 pl.pfs, sd.data_ptr() if stats else None)
            torch.cuda.synchronize()
            bufs = pl.host()
            problem = fk.planes_problem(bufs, ex.e, row.w, row.h, row.profile, pl.st)
            assert problem is None, (row.id, shape, halves, problem)
            assert fr.unchanged(), (row.id, shape, halves, "the source frames changed")
            if halves:      # frames that are halves by type take the half-input table kernel exactly when the table fits and no statistics are asked for
                took = cs.half_table_info(row.sc)["table_launches"] - before
                assert took == (1 if ce.half_table_fits(row.cfg) and not stats else 0), (row.id, shape, took)
            if stats:
                got = sd.cpu().numpy().reshape(NF, 3)
                for f in range(NF):
                    want = fk.expected_stats(o, row.cfg, widen_halves(ex.frames[f]) if halves else ex.frames[f], row.sc)
                    print("%s %s frame %d: {sum, min, max} %r, the oracle's %r" % (row.id, shape, f, tuple(got[f]), want))
                    problem = fk.stats_problem(got[f], want)
                    assert problem is None, (row.id, shape, halves, f, problem)
            if not halves:
                default = bufs if default is None else default
                assert all(np.array_equal(a, b) for a, b in zip(bufs, default)), (row.id, shape, "the default launch")


def decode_row(L, o, c, row):
    import torch
    ex = ce.frame_expected(o, row.cfg, row.profile, row.w, row.h, row.sc)
    src = laid_out(L, ex.s, row.w, row.h, row.profile)
    for shape, tunes in shapes_of(row):
        cs = context(L, row.cfg, None, tuple(("grid_dec", v) if k == "grid_enc" else (k, v) for k, v in tunes))
        for halves in (False, True):
            out = FloatOut(NF, row.w, row.h, dtype=np.float16 if halves else np.float32)
            (cs.decode_frames_device_f16 if halves else cs.decode_frames_device)(src.ptrs, src.st, src.pfs, NF, row.w, row.h, row.profile, row.sc,
                                                                                 out.ptr, out.fs)
            torch.cuda.synchronize()
            got = out.frames()
            want = ce.narrowed(ex.d) if halves else ex.d
            bad = differ(got.view(np.uint16) if halves else got, want)
            assert not bad.any(), (row.id, shape, halves, "%d values differ, the first at %r" % (int(bad.sum()), tuple(np.argwhere(bad)[0])))
    assert src.unchanged(), (row.id, "a source plane changed")


def light_row(L, o, c, row):
    ex = ce.frame_expected(o, row.cfg, row.profile, row.w, row.h, row.sc)
    src = laid_out(L, ex.s, row.w, row.h, row.profile)
    if not ce.light_accepted(row.cfg):
        buf = ll.light_buf(NF)
        refused(L, c, lambda: c.planes_light_level_frames_device(src.ptrs, src.st, src.pfs, NF, row.w, row.h, row.profile, row.sc, 1.0, buf.data_ptr()),
                lambda: bool((buf == OUT_FILL).all()) and src.unchanged(), (row.id,))
        # ... and the context goes on: the decode call takes the same planes
        out = FloatOut(NF, row.w, row.h)
        c.decode_frames_device(src.ptrs, src.st, src.pfs, NF, row.w, row.h, row.profile, row.sc, out.ptr, out.fs)
        assert not differ(out.frames(), ex.d).any(), (row.id, "the decode call after the refusal")
        return
    want = ll.model_frames(ex.d, 1.0)
    for shape, tunes in shapes_of(row):
        got = ll.planes_light(context(L, row.cfg, None, tunes), src, row.sc, 1.0)
        assert np.array_equal(got, want), (row.id, shape, got, want)
    assert src.unchanged(), (row.id, "a source plane changed")


def frame_call(family, c, fr, sc, given, block, form):
    if family == "distortion":
        return dist(c, fr, sc, given, form)
    return (dist_map if family == "distortion_map" else mom_map)(c, fr, sc, given, block, form)


def measuring_row(L, o, c, row):
    import torch
    family, w, h, profile = row.call, row.w, row.h, row.profile
    for halves in (False, True):
        form = "f16" if halves else "packed"
        ex = ce.frame_expected(o, row.cfg, profile, w, h, row.sc, halves)
        fr = Frames(ex.frames, dtype=np.float16 if halves else np.float32)
        e = laid_out(L, ex.e, w, h, profile)
        if ce.measuring_lm(row.cfg, halves, family) is None:
            block = ce.BLOCKS[family][0]
            buf = words_buf(NF * 15 * (-(-w // (block or w))) * (-(-h // (block or h))))
            fn = getattr(c, family + "_frames_device" + ("_f16" if halves else ""))
            refused(L, c, lambda: fn(fr.ptr, fr.fs, NF, w, h, row.sc, profile, e.ptrs, e.st, e.pfs, *(() if block is None else (block,)), buf.data_ptr()),
                    lambda: bool((buf == OUT_FILL).all()), (row.id, halves))
            # ... and the context goes on: the encode call takes the same frames
            pl = Planes(L, w, h, profile, NF, strides=fk.wide_layout(w, h, profile))
            (c.encode_frames_device_f16 if halves else c.encode_frames_device)(fr.ptr, fr.fs, NF, w, h, row.sc, profile, pl.ptrs, pl.st, pl.pfs, None)
            torch.cuda.synchronize()
            problem = fk.planes_problem(pl.host(), ex.e, w, h, profile, pl.st)
            assert problem is None, (row.id, halves, "the encode call after the refusal", problem)
            continue
        for block in ce.BLOCKS[family]:
            gv = ce.given(o, row, block, halves)
            g = laid_out(L, gv[0], w, h, profile)
            default = None
            for shape, tunes in shapes_of(row):
                cs = context(L, row.cfg, None, tunes)
                front_end_asserted(cs, row.cfg, row.sc, (row.id, shape))
                before = cs.half_table_info(row.sc)["table_launches"]
                got = frame_call(family, cs, fr, row.sc, g, block, form)
                assert np.array_equal(got, gv[1]), (row.id, halves, block, shape, got, gv[1])
                default = got if default is None else default
                assert np.array_equal(got, default), (row.id, halves, block, shape, "the default launch")
                pk.own_planes_measure_nothing(family, frame_call(family, cs, fr, row.sc, e, block, form), (row.id, halves, block, shape))
                assert cs.half_table_info(row.sc)["table_launches"] == before, (row.id, "a measuring launch counted as an encode launch")
            assert g.unchanged(), (row.id, halves, block, "a given plane changed")
        assert fr.unchanged() and e.unchanged(), (row.id, halves, "an input changed")


@pytest.mark.parametrize("row", [pytest.param(r, id=r.id) for r in FRAME_ROWS])
def test_frame_rows(L, oracle_mod, row):
    c = context(L, row.cfg)
    if row.call == "encode":
        encode_row(L, oracle_mod, c, row)
    elif row.call == "decode":
        decode_row(L, oracle_mod, c, row)
    elif row.call == "light":
        light_row(L, oracle_mod, c, row)
    else:
        measuring_row(L, oracle_mod, c, row)


# ---- 2. two quantizers
ACCEPTED_SOURCE = ce.PQ12_8      # the source every target of a refused pair takes (P1, and 8 bits of colour in the place of 10, 11, 12 or 16)


def half_call(c, src, src_sc, dst, dst_sc):
    c.transcode_half_frames_device(src.ptrs, src.st, src.pfs, src.profile, src_sc, src.nf, src.w, src.h, dst.ptrs, dst.st, dst.pfs, dst.profile, dst_sc,
                                   None)


def plane_call(family, c, src, src_sc, given, dst_sc, block):
    if family == "distortion":
        return measure(c, src, src_sc, given, dst_sc)
    return (tmap if family == "distortion_map" else tmom)(c, src, src_sc, given, dst_sc, block)


def written(L, c, row, src, stats=False):
    """one k_transcode or k_transcode_half launch into sentinel-filled planes in the wide layout: (Planes, host buffers, statistics)"""
    import torch
    tw, th = ce.target_size(row)
    if row.family == "transcode":
        out = transcoded(c, L, src, row.src_sc, row.dp, row.dst_sc, strides=fk.wide_layout(tw, th, row.dp), stats=stats)
        return out if stats else out + (None,)
    dst = Planes(L, tw, th, row.dp, NF, strides=fk.wide_layout(tw, th, row.dp))
    half_call(c, src, row.src_sc, dst, row.dst_sc)
    torch.cuda.synchronize()
    return dst, dst.host(), None


def refused_plane_row(L, o, row):
    import torch
    c = context(L, row.dcfg, row.scfg)
    src = laid_out(L, ce.source_planes(row.scfg, row.sp, row.w, row.h), row.w, row.h, row.sp)
    tw, th = ce.target_size(row)
    given = Planes(L, tw, th, row.dp, NF, strides=fk.wide_layout(tw, th, row.dp))
    block = ce.BLOCKS.get(row.family, (None,))[0]
    if row.family in ("transcode", "half"):
        call = (lambda: half_call(c, src, row.src_sc, given, row.dst_sc)) if row.family == "half" else \
            (lambda: c.transcode_frames_device(src.ptrs, src.st, src.pfs, row.sp, row.src_sc, NF, row.w, row.h, given.ptrs, given.st, given.pfs, row.dp,
                                               row.dst_sc, None))
        refused(L, c, call, given.unchanged, (row.id,))
    else:
        buf = words_buf(NF * (-(-row.w // (block or row.w))) * (-(-row.h // (block or row.h))) * 15)
        tail = () if block is None else (block,)
        fn = {"distortion": c.transcode_distortion_frames_device, "distortion_map": c.transcode_distortion_map_frames_device,
              "moments_map": c.transcode_moments_map_frames_device}[row.family]
        refused(L, c, lambda: fn(src.ptrs, src.st, src.pfs, row.sp, row.src_sc, NF, row.w, row.h, given.ptrs, given.st, given.pfs, row.dp, row.dst_sc,
                              *tail, buf.data_ptr()),
                lambda: bool((buf == OUT_FILL).all()) and given.unchanged(), (row.id,))
    assert src.unchanged(), (row.id, "a source plane changed")
    # the same context completes an accepted call: the same target from a source it takes, held to the oracle
    ok = row._replace(id=row.id + "-then-accepted", scfg=ACCEPTED_SOURCE, src_sc=1.0, dst_sc=ce.scalings(ACCEPTED_SOURCE, row.dcfg)[0][1])
    assert ce.row_accepted(ok), ok.id
    c.set_source_quantizer(*ok.scfg, L.build_lut(ok.scfg[0], ok.scfg[1], ok.scfg[4], ok.scfg[5]))
    try:
        accepted_plane_row(L, o, ok, c, shapes=False)
    finally:
        c.set_source_quantizer(*row.scfg, L.build_lut(row.scfg[0], row.scfg[1], row.scfg[4], row.scfg[5]))
    torch.cuda.synchronize()


def accepted_plane_row(L, o, row, c0=None, shapes=True):
    ex = ce.plane_expected(o, row)
    tw, th = ce.target_size(row)
    src = laid_out(L, ex.s, row.w, row.h, row.sp)
    default = {}
    for shape, tunes in (shapes_of(row) if shapes else [("default", ())]):
        c = c0 if c0 is not None else context(L, row.dcfg, row.scfg, tunes)
        front_end_asserted(c, row.dcfg, row.dst_sc, (row.id, shape))
        if row.family in ("transcode", "half"):
            stats = row.family == "transcode" and shape == "default" and alternate(row.sp + row.dp, (row.w, row.h), ce.PLANE_SIZES)
            dst, bufs, got = written(L, c, row, src, stats)
            problem = fk.planes_problem(bufs, ex.e, tw, th, row.dp, dst.st)
            assert problem is None, (row.id, shape, problem)
            assert all(np.array_equal(a, b) for a, b in zip(bufs, default.setdefault(None, bufs))), (row.id, shape, "the default launch")
            if stats:   # min and max bit for bit the encode call's on the oracle's decoded frames, the sum the oracle's within 1e-4
                enc = encode(c, L, Frames(ex.d), row.dst_sc, row.dp, stats=True)[2]
                for f in range(NF):
                    want = (fk.expected_stats(o, row.dcfg, ex.d[f], row.dst_sc)[0], enc[f][1], enc[f][2])
                    print("%s frame %d: {sum, min, max} %r, the encode call's %r, the oracle's sum %r" % (row.id, f, tuple(got[f]), tuple(enc[f]), want[0]))
                    problem = fk.stats_problem(got[f], want)
                    assert problem is None, (row.id, f, problem)
            continue
        e = laid_out(L, ex.e, tw, th, row.dp)
        for block in ce.BLOCKS[row.family]:
            gv = ce.given(o, row, block)
            g = laid_out(L, gv[0], tw, th, row.dp)
            got = plane_call(row.family, c, src, row.src_sc, g, row.dst_sc, block)
            assert np.array_equal(got, gv[1]), (row.id, shape, block, got, gv[1])
            assert np.array_equal(got, default.setdefault(block, got)), (row.id, shape, block, "the default launch")
            pk.own_planes_measure_nothing(row.family, plane_call(row.family, c, src, row.src_sc, e, row.dst_sc, block), (row.id, shape, block))
            assert g.unchanged(), (row.id, shape, block, "a given plane changed")
        assert e.unchanged(), (row.id, shape, "a given plane changed")
    assert src.unchanged(), (row.id, "a source plane changed")


@pytest.mark.parametrize("row", [pytest.param(r, id=r.id) for r in PLANE_ROWS])
def test_plane_rows(L, oracle_mod, row):
    if ce.row_accepted(row):
        accepted_plane_row(L, oracle_mod, row)
    else:
        refused_plane_row(L, oracle_mod, row)
