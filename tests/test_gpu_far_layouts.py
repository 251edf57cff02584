"""Every device entry point that takes a frame stride or plane frame strides, on frames and code planes that lie beyond 2^31 and 2^32
elements or bytes of the pointers it is given -- needs an MI355X.

The layouts, the lead that keeps a 32-bit address inside the allocation, the matrix and the expectations are
tests/support/far_layouts.py's; tests/test_far_layouts_host.py shows without a GPU that every row fails a kernel that narrows the frame
term or the row term.  Here each row runs the call once and holds what it delivers to the ORACLE (numpy for the words) bit for bit --
never to a compact-layout call of the library --, the far inputs to what they were over their whole allocation (looked at on the device
in pieces of 256 MiB) and the far outputs to "nothing but the samples was written".  Buffers are sparse: filled with the sentinel on the
device, the samples copied piecewise.  At most 24 GiB are live at once; a test skips only when the device reports less free memory than
it needs.  Refusals that must still refuse keep every argument inside real allocations."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from lumahdrv_amd.capi import LumaHipError  # noqa: E402
from tests.support import device as dv  # noqa: E402
from tests.support import far_layouts as fl  # noqa: E402
from tests.support import frame_kernels as fk  # noqa: E402
from tests.support import light_level as ll  # noqa: E402
from tests.support import planes_measure as pm  # noqa: E402
from tests.support.decode_kernels import differ  # noqa: E402
from tests.support.device import L  # noqa: E402,F401
from tests.support.display import DISPLAY_SETS, check_rgba  # noqa: E402
from tests.support.host import ERR_ARG, GUARD, OUT_FILL, SENTINEL, map_words, nwords  # noqa: E402
from tests.support.moments import mom_nwords, mom_words  # noqa: E402
from tests.support.transcode_half import box  # noqa: E402
from tests.support.transcode_moments import tmom  # noqa: E402

pytestmark = pytest.mark.gpu

ROWS = fl.matrix()
HEADROOM = 2 * fl.GIB      # beside a row's far operands: its compact operands, the pieces the sentinel checks look at, torch's own


@pytest.fixture(autouse=True)
def _release():
    yield
    import torch
    torch.cuda.empty_cache()


def _room(nbytes):
    free = fl.free_bytes()
    if free < nbytes + HEADROOM:
        pytest.skip("%.1f GiB of device memory free, the row needs %.1f" % (free / fl.GIB, (nbytes + HEADROOM) / fl.GIB))


_ctx = {}


def context(L, row):
    """a context under the row's quantizer (source and target alike) in the row's launch shape, made once"""
    cfg = fl.cfg_of(row.cs, row.profile)
    key = (cfg, row.shape)
    if key not in _ctx:
        c = dv.ctx(L, cfg, src_cfg=cfg)
        if row.shape == "two":
            for k, v in (("block", 64), ("grid_enc", 2), ("grid_dec", 2)):
                c.tune(k, v)
        elif row.shape == "1024":
            c.tune("block", 1024)
        _ctx[key] = c
    return _ctx[key]


# ---- operands
def in_frames(row, kind, frames):
    dt = np.float16 if fl.halves_of(row) else np.float32
    with np.errstate(over="ignore"):
        frames = frames.astype(dt)
    if kind == "compact":
        return dv.Frames(frames, dt)
    if kind == "planar3":
        return fl.FarPlanar(frames, row.nf, row.w, row.h, dt)
    return fl.FarFrames(frames, dt)


def out_frames(row, kind):
    dt = np.uint16 if fl.halves_of(row) else np.float32
    if kind == "compact":
        return dv.FloatOut(row.nf, row.w, row.h, dt)
    if kind == "planar3":
        return fl.FarPlanar(None, row.nf, row.w, row.h, dt)
    return fl.FarFloatOut(row.nf, row.w, row.h, dt, rot=(kind == "rot"))


def in_planes(L, row, kind, frames, w, h):
    if kind == "compact":
        return dv.from_frames(L, frames, w, h, row.profile, padding="sentinel")
    return fl.FarPlanes(L, w, h, row.profile, row.nf, fill_frames=frames, kind=kind)


def out_planes(L, row, kind, w, h):
    if kind == "compact":
        return dv.Planes(L, w, h, row.profile, row.nf)
    return fl.FarPlanes(L, w, h, row.profile, row.nf, kind=kind)


def colour_ptrs(fr, esz):
    """the three colour-plane pointers of frames in either kind of buffer"""
    return fr.plane_ptrs if hasattr(fr, "plane_ptrs") else [fr.ptr + k * fr.n * esz for k in range(3)]


def frames_arg(row, fr):
    return colour_ptrs(fr, 2 if fl.halves_of(row) else 4) if row.form.startswith("planar") else fr.ptr


def planes_read(pl, tag):
    """the frames of tight planes a call wrote, after checking that it wrote nothing else"""
    if isinstance(pl, fl.FarPlanes):
        assert pl.only_samples_written(), tag + ("a byte outside the samples was written",)
        return pl.host_frames()
    bufs = pl.host()
    assert pl.gaps_intact(bufs), tag + ("a byte outside the samples was written",)
    return fl.tight([pl.frame(bufs, f) for f in range(pl.nf)], pl.w, pl.h, pl.profile)


def frames_read(out, tag):
    if isinstance(out, dv.FloatOut):
        return out.frames()
    assert out.only_samples_written(), tag + ("a byte outside the frames was written",)
    return out.frames()


def same_frames(got, want, tag):
    want = np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, tag + (got.dtype, got.shape, want.dtype, want.shape)
    bad = differ(got, want)
    assert not bad.any(), tag + ("%d values differ, the first at %r" % (int(bad.sum()), tuple(int(v) for v in np.argwhere(bad)[0])),)


def same_planes(got, want, tag):
    for f, (a, b) in enumerate(zip(got, want)):
        for p in range(3):
            assert np.array_equal(a[p], b[p]), tag + (f, p, "%d bytes of this plane differ" % int(np.count_nonzero(a[p] != b[p])))


def same_stats(o, row, got, frames, tag):
    cfg = fl.cfg_of(row.cs, row.profile)
    for f in range(row.nf):
        prob = fk.stats_problem(got[f], fk.expected_stats(o, cfg, frames[f], 1.0))
        assert prob is None, tag + (f, prob)


def stats_of(row):
    return dv.stats_buf(row.nf) if row.stats else None


def _sptr(sd):
    return sd.data_ptr() if sd is not None else None


def _sync():
    import torch
    torch.cuda.synchronize()


def rows_of(*groups):
    return [pytest.param(r, id=r.id) for r in ROWS if r.group in groups]


# ---- 1. encode
@pytest.mark.parametrize("row", rows_of("encode"))
def test_encode(L, oracle_mod, row):
    _room(fl.live_bytes(row))
    tag = (row.id,)
    inp = fl.true_inputs(oracle_mod, row)
    exp = fl.expectation(oracle_mod, row, inp)
    c = context(L, row)
    fr = in_frames(row, row.a, inp.frames)
    pl = out_planes(L, row, row.b, row.w, row.h)
    sd = stats_of(row)
    getattr(c, "encode_frames_device" + fl.SUFFIX[row.form])(frames_arg(row, fr), fr.fs, row.nf, row.w, row.h, 1.0, row.profile, pl.ptrs, pl.st,
                                                             pl.pfs, _sptr(sd))
    _sync()
    same_planes(planes_read(pl, tag), exp, tag)
    assert fr.unchanged(), tag + ("the frames changed",)
    if sd is not None:
        same_stats(oracle_mod, row, sd.cpu().numpy().reshape(row.nf, 3), inp.frames, tag)


# ---- 2. decode
@pytest.mark.parametrize("row", rows_of("decode"))
def test_decode(L, oracle_mod, row):
    _room(fl.live_bytes(row))
    tag = (row.id,)
    inp = fl.true_inputs(oracle_mod, row)
    exp = fl.expectation(oracle_mod, row, inp)
    c = context(L, row)
    pl = in_planes(L, row, row.a, inp.planes_a, row.w, row.h)
    out = out_frames(row, row.b)
    args = (pl.ptrs, pl.st, pl.pfs, row.nf, row.w, row.h, row.profile, 1.0)
    if row.form == "rotating":
        c.decode_frames_device_rotating(*args, out.rot, out.fs)
    elif row.form.startswith("planar"):
        getattr(c, "decode_frames_device" + fl.SUFFIX[row.form])(*args, colour_ptrs(out, out.esz), out.fs)
    else:
        getattr(c, "decode_frames_device" + fl.SUFFIX[row.form])(*args, out.ptr, out.fs)
    _sync()
    same_frames(frames_read(out, tag), exp, tag)
    assert pl.unchanged(), tag + ("the planes changed",)


# ---- ... and the display form
@pytest.mark.parametrize("row", rows_of("display"))
def test_display_decode(L, oracle_mod, row):
    import torch
    _room(fl.live_bytes(row))
    tag = (row.id,)
    o, nf, w, h = oracle_mod, row.nf, row.w, row.h
    inp = fl.true_inputs(o, row)
    ts = fl.display_ts(o, row, inp)
    do_tmo, ldr_sim, exposure, gamma = DISPLAY_SETS[row.block]
    c = context(L, row)
    pl = in_planes(L, row, row.a, inp.planes_a, w, h)
    floats = dv.FloatOut(nf, w, h)
    if row.b == "fardisp":
        img = fl.FarDisplay(nf, w, h)
        ptr, pitch, dfs = img.ptr, img.st, img.fs
    else:
        pitch = 4 * w + 16
        dfs = h * pitch + 64
        img = torch.full((nf * dfs,), SENTINEL, dtype=torch.uint8, device=dv.dev())
        ptr = img.data_ptr()
    c.decode_display_frames_device(pl.ptrs, pl.st, pl.pfs, nf, w, h, row.profile, 1.0, ptr, pitch, dfs, exposure, gamma, do_tmo, ldr_sim,
                                   rgb_ptr=floats.ptr, frame_stride=floats.fs)
    _sync()
    if row.b == "fardisp":
        assert img.only_samples_written(), tag + ("a byte outside the image rows was written",)
        images = img.images()
    else:
        a = img.cpu().numpy().reshape(nf, dfs)
        rows_ = a[:, :h * pitch].reshape(nf, h, pitch)
        assert np.all(a[:, h * pitch:] == SENTINEL) and np.all(rows_[:, :, 4 * w:] == SENTINEL), tag + ("a byte outside the image rows was written",)
        images = [np.ascontiguousarray(rows_[f, :, :4 * w]).reshape(h, w, 4) for f in range(nf)]
    check_rgba(np.concatenate(images), np.concatenate(ts), tag)      # (the frames one above the other; the rule is display.py's, unchanged)
    same_frames(floats.frames(), fl.oracle_decode(o, fl.cfg_of(row.cs, row.profile), inp.planes_a, row.profile, w, h), tag)
    assert pl.unchanged(), tag + ("the planes changed",)


# ---- 3. transcode and transcode-half
@pytest.mark.parametrize("row", rows_of("transcode"))
def test_transcode(L, oracle_mod, row):
    _room(fl.live_bytes(row))
    tag = (row.id,)
    o = oracle_mod
    inp = fl.true_inputs(o, row)
    exp = fl.expectation(o, row, inp)
    c = context(L, row)
    tw, t_h = fl.dims_of(row, "planes_b")
    src = in_planes(L, row, row.a, inp.planes_a, row.w, row.h)
    dst = out_planes(L, row, row.b, tw, t_h)
    sd = stats_of(row)
    call = c.transcode_half_frames_device if row.entry == "half" else c.transcode_frames_device
    call(src.ptrs, src.st, src.pfs, row.profile, 1.0, row.nf, row.w, row.h, dst.ptrs, dst.st, dst.pfs, row.profile, 1.0, _sptr(sd))
    _sync()
    same_planes(planes_read(dst, tag), exp, tag)
    assert src.unchanged(), tag + ("the source planes changed",)
    if sd is not None:
        d = fl.oracle_decode(o, fl.cfg_of(row.cs, row.profile), inp.planes_a, row.profile, row.w, row.h)
        same_stats(o, row, sd.cpu().numpy().reshape(row.nf, 3), box(d) if row.entry == "half" else d, tag)


# ---- 4. to 6. the measuring calls
def _words_buf(row):
    """(the buffer of a measuring call, the reader of its words)"""
    fam, nf, w, h, blk = fl.family_of(row), row.nf, row.w, row.h, row.block
    if fam == "distortion":
        return pm.frame_buf(nf), lambda b: pm.frame_words(b, nf)
    if fam == "distortion_map":
        return dv.map_buf(nwords(nf, w, h, blk)), lambda b: map_words(b, nf, w, h, blk)
    return dv.map_buf(mom_nwords(nf, w, h, blk)), lambda b: mom_words(b, nf, w, h, blk)


@pytest.mark.parametrize("row", rows_of("measure"))
def test_frame_fed_measures(L, oracle_mod, row):
    _room(fl.live_bytes(row))
    tag = (row.id,)
    inp = fl.true_inputs(oracle_mod, row)
    exp = fl.expectation(oracle_mod, row, inp)
    assert exp[..., 0].any(), tag + ("nothing to measure",)
    c = context(L, row)
    fr = in_frames(row, row.a, inp.frames)
    given = in_planes(L, row, row.b, inp.planes_b, row.w, row.h)
    buf, words = _words_buf(row)
    args = (frames_arg(row, fr), fr.fs, row.nf, row.w, row.h, 1.0, row.profile, given.ptrs, given.st, given.pfs)
    getattr(c, row.entry + "_frames_device" + fl.SUFFIX[row.form])(*args, *(() if row.block is None else (row.block,)), buf.data_ptr())
    _sync()
    got = words(buf)
    assert np.array_equal(got, exp), tag + ("%d words differ" % int(np.count_nonzero(got != exp)),)
    assert fr.unchanged() and given.unchanged(), tag + ("an input changed",)


@pytest.mark.parametrize("row", rows_of("tmeasure"))
def test_transcode_measures(L, oracle_mod, row):
    _room(fl.live_bytes(row))
    tag = (row.id,)
    inp = fl.true_inputs(oracle_mod, row)
    exp = fl.expectation(oracle_mod, row, inp)
    assert exp[..., 0].any(), tag + ("nothing to measure",)
    c = context(L, row)
    src = in_planes(L, row, row.a, inp.planes_a, row.w, row.h)
    given = in_planes(L, row, row.b, inp.planes_b, row.w, row.h)
    if row.entry == "tdistortion":
        got = dv.measure(c, src, 1.0, given, 1.0)
    elif row.entry == "tdistortion_map":
        got = dv.tmap(c, src, 1.0, given, 1.0, row.block)
    else:
        got = tmom(c, src, 1.0, given, 1.0, row.block)
    assert np.array_equal(got, exp), tag + ("%d words differ" % int(np.count_nonzero(got != exp)),)
    assert src.unchanged() and given.unchanged(), tag + ("an input changed",)


@pytest.mark.parametrize("row", rows_of("pmeasure"))
def test_plane_to_plane_measures(L, oracle_mod, row):
    _room(fl.live_bytes(row))
    tag = (row.id,)
    inp = fl.true_inputs(oracle_mod, row)
    exp = fl.expectation(oracle_mod, row, inp)
    assert exp[..., 0].any(), tag + ("nothing to measure",)
    c = context(L, row)
    a = in_planes(L, row, row.a, inp.planes_a, row.w, row.h)
    b = in_planes(L, row, row.b, inp.planes_b, row.w, row.h)
    if row.entry == "pdistortion":
        got = pm.pdist(c, a, b)
    elif row.entry == "pdistortion_map":
        got = pm.pmap(c, a, b, row.block)
    else:
        got = pm.pmom(c, a, b, row.block)
    assert np.array_equal(got, exp), tag + ("%d words differ" % int(np.count_nonzero(got != exp)),)
    assert a.unchanged() and b.unchanged(), tag + ("an input changed",)


# ---- 7. the light level
@pytest.mark.parametrize("row", rows_of("light"))
def test_light_level(L, oracle_mod, row):
    _room(fl.live_bytes(row))
    tag = (row.id,)
    inp = fl.true_inputs(oracle_mod, row)
    exp = fl.expectation(oracle_mod, row, inp)
    c = context(L, row)
    if row.entry == "plight":
        src = in_planes(L, row, row.a, inp.planes_a, row.w, row.h)
        got = ll.planes_light(c, src, 1.0, fl.LIGHT_SCALE)
    else:
        src = in_frames(row, row.a, inp.frames)
        buf = ll.light_buf(row.nf)
        getattr(c, "light_level_frames_device" + fl.SUFFIX[row.form])(frames_arg(row, src), src.fs, row.nf, row.w, row.h, fl.LIGHT_SCALE, buf.data_ptr())
        _sync()
        got = ll.light_words(buf, row.nf)
    assert np.array_equal(got, exp), tag + (got, exp)
    assert src.unchanged(), tag + ("the input changed",)


# ---- 8. the stand-alone transform and the generator
@pytest.mark.parametrize("row", rows_of("frames"))
def test_transform_and_generator(L, oracle_mod, row):
    _room(fl.live_bytes(row))
    tag = (row.id,)
    inp = fl.true_inputs(oracle_mod, row)
    exp = fl.expectation(oracle_mod, row, inp)
    c = context(L, row)
    if row.entry == "transform":
        buf = fl.FarFrames(inp.frames)
        c.transform_frames_device(buf.ptr, buf.fs, row.nf, row.w, row.h, True, 1.0)
    else:
        buf = fl.FarFloatOut(row.nf, row.w, row.h)
        c.synth_frames_device(buf.ptr, buf.fs, row.nf, row.w, row.h)
    _sync()
    assert buf.only_samples_written(), tag + ("a byte outside the frames was written",)
    got = np.stack([a.view(np.float32).reshape(3, row.h, row.w) for a in buf.samples()])
    same_frames(got, exp, tag)


# ---- 9. refusals that must still refuse: nothing launched, the output as it was, the context usable
def _row(entry, symbol, a, b, profile, nf=3):
    """a row of REFUSAL_SIZE under PQ-11 Lu'v', as the matrix would write it"""
    w, h = fl.REFUSAL_SIZE
    return fl.Row("refusal", "refusal", entry, symbol, "packed" if entry == "distortion" else None, a, b, w, h, "luv", profile, False, None, "default", nf)


def _refused(call):
    with pytest.raises(LumaHipError) as e:
        call()
    assert e.value.code == ERR_ARG, str(e.value)
    _sync()


def test_refused_words_inside_far_frame_2(L, oracle_mod):
    row = _row("distortion", "lumahip_distortion_frames_device", "far", "compact", 2)
    _room(fl.live_bytes(row))
    a = fl.refusal_args("words_in_far_frame_2")
    inp = fl.true_inputs(oracle_mod, row)
    c = context(L, row)
    fr = in_frames(row, "far", inp.frames)
    given = in_planes(L, row, "compact", inp.planes_b, row.w, row.h)
    assert (fr.fs, fr.ptr - fr.t.data_ptr()) == (a["fl"].fs, a["ptr"])
    out = fr.t.data_ptr() + a["out"]
    assert fr.ptr + 2 * fr.fs * 4 < out and out + a["out_bytes"] <= fr.ptr + (2 * fr.fs + fr.n) * 4 <= fr.t.data_ptr() + fr.t.numel()
    _refused(lambda: c.distortion_frames_device(fr.ptr, fr.fs, 3, row.w, row.h, 1.0, 2, given.ptrs, given.st, given.pfs, out))
    assert fr.unchanged() and given.unchanged()
    assert np.array_equal(dv.dist(c, fr, 1.0, given), fl.expectation(oracle_mod, row, inp))


def test_refused_words_inside_the_last_row_of_a_wide_plane(L, oracle_mod):
    row = _row("plight", "lumahip_planes_light_level_frames_device", "wide", None, 3, nf=1)
    _room(fl.live_bytes(row))
    a = fl.refusal_args("words_in_last_wide_row")
    inp = fl.true_inputs(oracle_mod, row)
    c = context(L, row)
    pl = in_planes(L, row, "wide", inp.planes_a, row.w, row.h)
    assert pl.pl == a["pl"]
    out = pl.t.data_ptr() + a["out"]
    assert out % 8 == 0 and out + a["out_bytes"] <= pl.t.data_ptr() + pl.t.numel()
    _refused(lambda: c.planes_light_level_frames_device(pl.ptrs, pl.st, pl.pfs, 1, row.w, row.h, 3, 1.0, fl.LIGHT_SCALE, out))
    assert pl.unchanged()
    assert np.array_equal(ll.planes_light(c, pl, 1.0, fl.LIGHT_SCALE), fl.expectation(oracle_mod, row, inp))


def test_refused_target_planes_over_far_frame_2_of_the_source(L, oracle_mod):
    row = _row("transcode", "lumahip_transcode_frames_device", "far16", "compact", 2)
    _room(fl.live_bytes(row))
    a = fl.refusal_args("target_over_far_frame_2")
    inp = fl.true_inputs(oracle_mod, row)
    c = context(L, row)
    src = in_planes(L, row, "far16", inp.planes_a, row.w, row.h)
    assert src.pl == a["pl"]
    base, end = src.t.data_ptr(), src.t.data_ptr() + src.t.numel()
    dst = [base + d for d in a["dst"]]
    assert all(base <= dst[p] and dst[p] + a["ext"][p] <= end for p in range(3))
    _refused(lambda: c.transcode_frames_device(src.ptrs, src.st, src.pfs, 2, 1.0, 3, row.w, row.h, dst, a["st"], a["tpfs"], 2, 1.0, None))
    assert src.unchanged()
    good = out_planes(L, row, "compact", row.w, row.h)
    c.transcode_frames_device(src.ptrs, src.st, src.pfs, 2, 1.0, 3, row.w, row.h, good.ptrs, good.st, good.pfs, 2, 1.0, None)
    _sync()
    same_planes(planes_read(good, (row.id,)), fl.expectation(oracle_mod, row, inp), (row.id,))


def test_refused_frame_stride_below_a_wide_plane(L, oracle_mod):
    row = _row("plight", "lumahip_planes_light_level_frames_device", "wide", None, 3, nf=2)
    _room(fl.live_bytes(row))
    a = fl.refusal_args("pfs_below_wide_plane")
    c = context(L, row)
    frames = fl.code_planes(fl.cfg_of("luv", 3), 3, row.w, row.h, 3)[:2]
    pl = fl.FarPlanes(L, row.w, row.h, 3, 2, fill_frames=frames, kind="wide")
    assert pl.pl == a["pl"] and all(a["pfs"][p] < pl.pl.rows[p] * pl.st[p] for p in range(3))
    buf = ll.light_buf(2)
    _refused(lambda: c.planes_light_level_frames_device(pl.ptrs, pl.st, a["pfs"], 2, row.w, row.h, 3, 1.0, fl.LIGHT_SCALE, buf.data_ptr()))
    assert bool((buf == OUT_FILL).all()) and buf.numel() == 2 * ll.WORDS + GUARD and pl.unchanged()
    # the context still works, on the same planes laid out as they are
    got = ll.planes_light(c, pl, 1.0, fl.LIGHT_SCALE)
    want = ll.model_frames(fl.oracle_decode(oracle_mod, fl.cfg_of("luv", 3), frames, 3, row.w, row.h), fl.LIGHT_SCALE)
    assert np.array_equal(got, want)
