"""lumahip_decode_display_frames_device, every kernel it can launch -- needs an MI355X.

Each case holds the RGBA image to the float64 transform of the oracle's decoded floats (tests/support/display.py check_rgba: equal, or
one code off within EPS of a rounding boundary and towards it; at most 1 % of the pixels that close), the float output bit for bit to
orc.decode, the sentinel bytes behind every RGBA row, between the frames and behind the last one, and the code planes to what they were.
The planes are the oracle's encode of three distinct frames with the out-of-range codes tests/golden/make_golden.py writes into its
decode fixtures, so NaN, inf and clamped values pass through the epilogue.  Every launch has three frames, an RGBA pitch of 4 w + 12
bytes, 20 bytes between the frames' images and 4 floats between the float frames.

Which k_decode<CS, SUB, VW | GL, DISP = true> a call launches follows from its arguments (lumahip_decode.hip decode_impl):
  four pixels per thread, table in LDS      test_display_matrix[*-64x32-lds]   w % 4 == 0, 16-byte aligned floats, frame stride % 4 == 0
  two pixels per thread, table in LDS       test_display_matrix[*-258x6-lds] (a ragged last tile, three tiles per row) and [*-6x4-lds]
  table in global memory (two pixels)       test_display_matrix[*-64x32-global]
for CS in Lu'v' (pq11_luv8 profiles 2, 3; pq8_luv8 profiles 0, 1), RGB (pq12_rgb 2, 3), XYZ (linear12_xyz 2, 3) and YCbCr (pq10_ycbcr10
2, 3), SUB = 4:2:0 (profiles 0, 2) or 4:4:4 (1, 3): 4 x 2 x 3 = 24 kernels.  The sample size is a kernel argument, not an instantiation.
The table leaves LDS under lumahip_tune "lds_table_max_kb" 0 only when it is longer than 16 KiB (lumahip_core.hip
upload_decode_tables), so the `global` cases run the same colour spaces with a 13-bit table (profiles 2 and 3: its codes need 16-bit
samples); they assert that the records left LDS with it (quantizer_info mode 4).
The YCbCr rows run with preScaling 20 and 65537 -- inside and outside the short-division range, the two copies of the unit's code
k_decode picks by XformConst::sc_mode -- and on a context whose quantizer owns the y table (`yt1`, the default: decode_impl then takes the
table's bytes off the LDS size, since the display kernels do not stage it) as well as under lumahip_tune "ycbcr_tables" 0 (`yt0`).
The four parameter sets of test_decode_display_transform go round the matrix, so that each meets every colour space.
  display only (rgb_dev NULL, frame stride 0)          test_display_only_equals_the_call_with_floats
  the persistent loop, frames changing inside it       test_two_workgroups_of_one_wave_give_the_same_bytes ("grid_dec" 2, "block" 64)
  inside an unordered section                          test_inside_an_unordered_section
  a larger frame, twice                                test_a_larger_frame_twice
  refused calls write nothing                          test_refused_calls_launch_nothing
The k_decode<CS_PACK, ., ., DISP = true> instantiations are reachable from no entry point and are not run.

The conditions on the inputs (tests/support/display.py informative: 200 distinct codes per channel, under 20 % of the pixels at 0 or
255) are asserted on the float64 reference of every case of 64x32 and 258x6 -- 6x4 has 72 samples per channel.  Where a case cannot
show 200 codes the bound is 80 % of what it can: under the LDR simulation (201 and 87 codes exist), with preScaling 65537 (the
quantizer's peak of 1000 / 65537 is all an image can hold: 39 codes under the first parameter set), with an 8-bit RGB table.

Measured on an MI355X (every case prints its figures): the exempt share is at most 0.99 %; in the matrix 22 codes of 62 cases differ
from floor(t), the farthest 7.5e-5 from its boundary; on the 1280 x 720 frames 11 (Lu'v'), 203 (YCbCr, tone curve) and 0 (8-bit RGB, LDR) codes per image, the farthest 1.13e-4 -- against
EPS = 7.0e-4, and where the numpy float32 evaluation of the same formula differs as well."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.golden.make_golden import CONFIGS  # noqa: E402
from tests.support.device import L, ctx, dev, from_frames  # noqa: E402,F401  (L is the module fixture)
from tests.support.display import (DISPLAY_SETS, EPS, MAX_EXEMPT, check_rgba, display_frames, display_t, exempt_share, informative,  # noqa: E402
                                   reachable_codes)  # noqa: E402
from tests.support.host import ERR_ARG, SENTINEL, same_bits  # noqa: E402

NF = 3
PITCH_PAD, FRAME_PAD, TAIL, FLOAT_PAD = 12, 20, 64, 4
GARBAGE = [0xFF, 0xFF, 0x00, 0x00, 0x34, 0x12, 0xFF, 0x7F]     # make_golden.py's decode fixtures: row 0 of every plane
SIZES = [(64, 32), (258, 6), (6, 4)]

# name -> (configuration, its 13-bit sibling for the table in global memory, preScaling per unit of exposure, how far the frames reach
# under the tone curve).  The frames reach `top` / exposure, which the preScaling takes to about 100 cd/m2 under the PQ tables and to
# 8300 of the linear table's 10000; under the tone curve the PQ tables take frames that reach 150 (display_frames), the linear table's
# 12 binades and YCbCr's mandated preScalings do not.
LUV, RGB, XYZ, YCC = 0, 1, 2, 3
SPACES = {
    "pq11_luv8": (CONFIGS["pq11_luv8"], (1, 13, LUV, 8, 1e4, 0.005), 100.0, 150.0),
    "pq8_luv8": (CONFIGS["pq8_luv8"], None, 100.0, 150.0),
    "pq12_rgb": (CONFIGS["pq12_rgb"], (1, 13, RGB, 8, 1e4, 0.005), 100.0, 150.0),
    "linear12_xyz": (CONFIGS["linear12_xyz"], (4, 13, XYZ, 8, 1e4, 0.005), 8000.0, 1.04),
    "pq10_ycbcr10": (CONFIGS["pq10_ycbcr10"], (1, 13, YCC, 10, 1000.0, 0.01), None, 1.04),
    "pq8_rgb": ((1, 8, RGB, 8, 1e4, 0.005), None, 100.0, 150.0),
}


def rows():
    """(id, space, profile, YCbCr preScaling or None, ycbcr_tables)"""
    out = []
    for name, profiles in (("pq11_luv8", (2, 3)), ("pq8_luv8", (0, 1)), ("pq12_rgb", (2, 3)), ("linear12_xyz", (2, 3))):
        out += [("%s-p%d" % (name, p), name, p, None, 1) for p in profiles]
    for yt in (1, 0):
        for sc in (20.0, 65537.0):
            out += [("pq10_ycbcr10-p%d-sc%g-yt%d" % (p, sc, yt), "pq10_ycbcr10", p, sc, yt) for p in (2, 3)]
    return out


def matrix():
    cases = []
    for r, row in enumerate(rows()):
        forms = [(w, h, "lds") for (w, h) in SIZES] + ([(64, 32, "global")] if SPACES[row[1]][1] is not None else [])
        for k, (w, h, form) in enumerate(forms):
            cases.append(pytest.param(row, w, h, form, (r + k) % 4, id="%s-%dx%d-%s" % (row[0], w, h, form)))
    return cases


def test_the_matrix_covers_what_the_docstring_says():
    """24 (colour space, subsampling, form) triples, and every parameter set on every colour space"""
    kernels, sets = set(), set()
    for c in matrix():
        row, w, h, form, k = c.values
        cs = SPACES[row[1]][0][2]
        vw = "global" if form == "global" else (4 if w % 4 == 0 else 2)
        kernels.add((cs, row[2] in (0, 2), vw))
        sets.add((cs, k))
    assert len(kernels) == 24 and len(sets) == 16


# ---- a case: contexts, inputs, the reference
_ctx, _orc = {}, {}


def context(L, cfg, tunes=()):
    """a context on torch's stream per (configuration, tunes), made once"""
    key = (cfg, tuple(tunes))
    if key not in _ctx:
        c = ctx(L, cfg)
        for name, v in tunes:
            c.tune(name, v)
        _ctx[key] = c
    return _ctx[key]


def oracle(o, L, cfg):
    if cfg not in _orc:
        _orc[cfg] = o.Oracle(*cfg)
        assert same_bits(L.build_lut(cfg[0], cfg[1], cfg[4], cfg[5]), _orc[cfg].mapping), "the library's table is not the oracle's"
    return _orc[cfg]


class Case:
    """NF frames under a configuration: the planes on the device, the oracle's floats and t per frame"""

    def __init__(self, L, o, cfg, profile, w, h, kset, ycc_sc=None, per_exposure=100.0, tmo_top=1.04, seed=0, nf=NF):
        self.do_tmo, self.ldr_sim, self.exposure, self.gamma = self.kset = DISPLAY_SETS[kset]
        self.cfg, self.profile, self.w, self.h, self.nf = cfg, profile, w, h, nf
        top = tmo_top if (self.do_tmo and not self.ldr_sim) else 1.04
        self.sc = float(np.float32(ycc_sc if ycc_sc is not None else per_exposure * (1.0 if self.ldr_sim else self.exposure) * 1.04 / top))
        self.peak = cfg[4] / self.sc / (1.1 if cfg[2] == XYZ else 1.0)      # (Z of white is 1.09)
        orc = oracle(o, L, cfg)
        # a frame of 24 pixels has 4 % of them next to a rounding boundary with the first such pixel: the inputs, not the cap, give way
        # (the float64 reference alone decides)
        for attempt in range(32):
            self.build(L, orc, np.random.default_rng(1000 * w + 10 * h + profile + 7 * kset + seed + 100000 * attempt), top)
            if exempt_share(np.concatenate(self.t)) <= MAX_EXEMPT:
                break

    def build(self, L, orc, rng, top):
        w, h, profile, nf = self.w, self.h, self.profile, self.nf
        frames = []
        inputs = display_frames(rng, nf, w, h, self.exposure, self.gamma, self.do_tmo, self.ldr_sim, self.peak, top)
        self.reach = min(self.peak, float(inputs.max()))
        for f in inputs:
            planes, st, _ = orc.encode(f.copy(), self.sc, profile)
            for p in planes:
                n = min(len(GARBAGE), p.shape[1])
                p[0, :n] = GARBAGE[:n]
            frames.append(planes)
        self.planes = from_frames(L, frames, w, h, profile, padding="sentinel")
        host = self.planes.host()
        self.floats = [orc.decode(self.planes.frame(host, f), self.planes.st, w, h, self.sc, profile) for f in range(nf)]
        self.t = [display_t(d, self.exposure, self.gamma, self.do_tmo, self.ldr_sim) for d in self.floats]

    def levels(self):
        """what limits the codes this case can show: the distinct values a decoded channel holds, the codes up to the largest input"""
        held = min(np.unique(np.stack(self.floats)[:, c]).size for c in range(3))
        return min(held, reachable_codes(self.exposure, self.gamma, self.do_tmo, self.ldr_sim, self.reach))

    def inputs_are_informative(self, tag):
        return informative(np.concatenate(self.t), self.exposure, self.gamma, self.do_tmo, self.ldr_sim, tag, self.levels())


class Outputs:
    """the RGBA buffer (rows pitch bytes apart, frames fs bytes apart, the sentinel everywhere, 4 bytes in front of the first frame so
    that the base is 4-byte aligned and no more) and the float buffer (frames 3 w h + FLOAT_PAD floats apart)"""

    def __init__(self, case, floats=True, pitch_pad=PITCH_PAD, frame_pad=FRAME_PAD):
        import torch
        w, h, nf = case.w, case.h, case.nf
        self.w, self.h, self.nf = w, h, nf
        self.pitch = 4 * w + pitch_pad
        self.fs = h * self.pitch + frame_pad
        self.rgba = torch.full((4 + nf * self.fs + TAIL,), SENTINEL, dtype=torch.uint8, device=dev())
        self.n3 = 3 * w * h
        self.ffs = self.n3 + FLOAT_PAD if floats else 0
        self.rgb = torch.full((4 * nf * self.ffs,), SENTINEL, dtype=torch.uint8, device=dev()) if floats else None

    @property
    def rgba_ptr(self):
        return self.rgba.data_ptr() + 4

    def call(self, c, case):
        import torch
        pl = case.planes
        c.decode_display_frames_device(pl.ptrs, pl.st, pl.pfs, case.nf, case.w, case.h, case.profile, case.sc, self.rgba_ptr, self.pitch,
                                       self.fs, case.exposure, case.gamma, case.do_tmo, case.ldr_sim,
                                       rgb_ptr=self.rgb.data_ptr() if self.rgb is not None else None, frame_stride=self.ffs)
        torch.cuda.synchronize()
        return self

    def images(self):
        """(nf, h, w, 4) uint8, after checking every byte outside the images"""
        a = self.rgba.cpu().numpy()
        assert np.all(a[:4] == SENTINEL) and np.all(a[4 + self.nf * self.fs:] == SENTINEL), "bytes in front of / behind the frames"
        fr = a[4:4 + self.nf * self.fs].reshape(self.nf, self.fs)
        assert np.all(fr[:, self.h * self.pitch:] == SENTINEL), "bytes between the frames"
        rws = fr[:, :self.h * self.pitch].reshape(self.nf, self.h, self.pitch)
        assert np.all(rws[:, :, 4 * self.w:] == SENTINEL), "bytes behind a row"
        return np.ascontiguousarray(rws[:, :, :4 * self.w]).reshape(self.nf, self.h, self.w, 4)

    def float_frames(self):
        """(nf, 3, h, w) float32, after checking the gaps"""
        a = self.rgb.cpu().numpy().reshape(self.nf, 4 * self.ffs)
        assert np.all(a[:, 4 * self.n3:] == SENTINEL), "bytes between the float frames"
        return np.ascontiguousarray(a[:, :4 * self.n3]).view(np.float32).reshape(self.nf, 3, self.h, self.w)

    def untouched(self):
        return bool((self.rgba == SENTINEL).all()) and (self.rgb is None or bool((self.rgb == SENTINEL).all()))


def held_to_the_reference(case, out, tag, floats=True):
    """the four checks of a case; returns (exempt share, codes that differ, farthest boundary distance of one) over its frames"""
    img = out.images()
    if floats:
        got = out.float_frames()
        for f in range(case.nf):
            assert same_bits(got[f], case.floats[f]), tag + (f, "the float output is not the oracle's")
    assert case.planes.unchanged(), tag + ("a code plane changed",)
    share, differ, far = check_rgba(np.concatenate(img), np.concatenate(case.t), tag)      # (the frames one above the other)
    print("%s: exempt share %.4f, %d codes differ, farthest %.2e from a boundary (EPS %.2e)" % ("-".join(str(x) for x in tag), share,
                                                                                               differ, far, EPS))
    return img


@pytest.mark.parametrize("row,w,h,form,kset", matrix())
def test_display_matrix(L, oracle_mod, row, w, h, form, kset):
    _, name, profile, ycc_sc, yt = row
    cfg, cfg13, per_exposure, tmo_top = SPACES[name]
    tunes = [] if yt else [("ycbcr_tables", 0)]
    if form == "global":
        cfg, tunes = cfg13, tunes + [("lds_table_max_kb", 0)]
    c = context(L, cfg, tunes)
    if form == "global":
        assert c.quantizer_info()["mode"] == 4          # the 13-bit table's records are in global memory, as the table is
    case = Case(L, oracle_mod, cfg, profile, w, h, kset, ycc_sc, per_exposure, tmo_top)
    tag = (row[0], w, h, form, kset)
    if (w, h) != (6, 4):
        case.inputs_are_informative(tag)
    held_to_the_reference(case, Outputs(case).call(c, case), tag)


# ---- the further cases: Lu'v' 4:2:0, YCbCr 4:4:4, RGB with 8-bit samples
FURTHER = [pytest.param("pq11_luv8", 2, None, 0, id="luv420"), pytest.param("pq10_ycbcr10", 3, 20.0, 1, id="ycbcr444"),
           pytest.param("pq8_rgb", 0, None, 3, id="rgb8")]


def further_case(L, o, name, profile, ycc_sc, kset, w, h, **kw):
    return Case(L, o, SPACES[name][0], profile, w, h, kset, ycc_sc, SPACES[name][2], SPACES[name][3], **kw)


@pytest.mark.parametrize("w,h", [(64, 32), (258, 6)])
@pytest.mark.parametrize("name,profile,ycc_sc,kset", FURTHER)
def test_display_only_equals_the_call_with_floats(L, oracle_mod, name, profile, ycc_sc, kset, w, h):
    """rgb_dev NULL, frame stride 0 (the vector width then comes from null plane pointers): the bytes of the call with a float output"""
    case = further_case(L, oracle_mod, name, profile, ycc_sc, kset, w, h)
    c = context(L, case.cfg)
    tag = (name, profile, w, h, "display only")
    case.inputs_are_informative(tag)
    both = held_to_the_reference(case, Outputs(case).call(c, case), tag + ("with floats",))
    only = held_to_the_reference(case, Outputs(case, floats=False).call(c, case), tag, floats=False)
    assert np.array_equal(only, both), tag


@pytest.mark.parametrize("w,h", [(258, 6), (64, 32)])
@pytest.mark.parametrize("name,profile,ycc_sc,kset", FURTHER)
def test_two_workgroups_of_one_wave_give_the_same_bytes(L, oracle_mod, name, profile, ycc_sc, kset, w, h):
    """"grid_dec" 2 and "block" 64: one row pair per tile, 27 (258x6) or 48 (64x32) tiles over three frames for two workgroups -- the
    persistent loop runs and changes frame inside it; the bytes of the default launch shape"""
    case = further_case(L, oracle_mod, name, profile, ycc_sc, kset, w, h)
    tag = (name, profile, w, h, "two workgroups")
    default = held_to_the_reference(case, Outputs(case).call(context(L, case.cfg), case), tag + ("default",))
    looped = held_to_the_reference(case, Outputs(case).call(context(L, case.cfg, [("grid_dec", 2), ("block", 64)]), case), tag)
    assert np.array_equal(looped, default), tag


@pytest.mark.parametrize("name,profile,ycc_sc,kset", FURTHER)
def test_inside_an_unordered_section(L, oracle_mod, name, profile, ycc_sc, kset):
    """the display decode takes no part in a section (include/lumahip.h: all other entry points keep using the context's stream): between
    begin_unordered(2) and end_unordered it gives the ordered call's bytes, ordered with torch's stream as before"""
    case = further_case(L, oracle_mod, name, profile, ycc_sc, kset, 64, 32)
    c = context(L, case.cfg)
    tag = (name, profile, "unordered")
    ordered = held_to_the_reference(case, Outputs(case).call(c, case), tag + ("ordered",))
    c.begin_unordered(2)
    try:
        inside = Outputs(case).call(c, case)
    finally:
        c.end_unordered()
    assert np.array_equal(held_to_the_reference(case, inside, tag), ordered), tag


@pytest.mark.parametrize("name,profile,ycc_sc,kset", FURTHER)
def test_a_larger_frame_twice(L, oracle_mod, name, profile, ycc_sc, kset):
    """one 1280 x 720 frame -- 57600 tiles' worth of pixels, more than the grid holds at once -- run twice: the same bytes"""
    case = further_case(L, oracle_mod, name, profile, ycc_sc, kset, 1280, 720, nf=1)
    c = context(L, case.cfg)
    tag = (name, profile, 1280, 720)
    case.inputs_are_informative(tag)
    first = held_to_the_reference(case, Outputs(case).call(c, case), tag + ("first",))
    second = held_to_the_reference(case, Outputs(case).call(c, case), tag + ("second",))
    assert np.array_equal(first, second), tag


def test_refused_calls_launch_nothing(L, oracle_mod):
    """every refused call returns LUMAHIP_ERR_ARG and leaves the RGBA buffer and the float buffer as they were"""
    import torch
    case = further_case(L, oracle_mod, "pq11_luv8", 2, None, 0, 64, 32)
    c = context(L, case.cfg)
    out = Outputs(case)
    pl, w, h = case.planes, case.w, case.h
    good = dict(w=w, rgba=out.rgba_ptr, pitch=out.pitch, fs=out.fs, gamma=2.2, rgb=out.rgb.data_ptr(), ffs=out.ffs)
    bad = [("an RGBA pointer misaligned by 2", dict(rgba=out.rgba_ptr + 2)), ("a pitch that is no multiple of 4", dict(pitch=out.pitch + 2)),
           ("a pitch below 4 w", dict(pitch=4 * w - 4)), ("an RGBA frame stride that is no multiple of 4", dict(fs=out.fs + 2)),
           ("gamma 0", dict(gamma=0.0)), ("a negative gamma", dict(gamma=-2.2)), ("a NaN gamma", dict(gamma=float("nan"))),
           ("a null RGBA pointer", dict(rgba=None)), ("an odd width", dict(w=w - 1)),
           ("a float pointer misaligned by 4", dict(rgb=out.rgb.data_ptr() + 4)), ("an odd float frame stride", dict(ffs=out.ffs + 1))]
    for what, change in bad:
        a = dict(good, **change)
        with pytest.raises(L.LumaHipError) as e:
            c.decode_display_frames_device(pl.ptrs, pl.st, pl.pfs, case.nf, a["w"], h, case.profile, case.sc, a["rgba"], a["pitch"], a["fs"],
                                           1.0, a["gamma"], 0, 0, rgb_ptr=a["rgb"], frame_stride=a["ffs"])
        assert e.value.code == ERR_ARG, what
        torch.cuda.synchronize()
        assert out.untouched(), what
    # binary16 frames and the rotating layout have no display output by design; the binding has no call that could ask for one
    held_to_the_reference(case, out.call(c, case), ("after the refused calls",))
