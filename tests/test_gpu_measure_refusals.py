"""What the measuring calls refuse, and in which words: the frame-fed calls (lumahip_distortion / _distortion_map / _moments_map
_frames_device, floats and halves, packed and planar), the plane-fed ones (lumahip_transcode_distortion / _distortion_map / _moments_map),
the plane-to-plane ones (lumahip_planes_distortion / _distortion_map / _moments_map), the content light level of frames and of planes,
and the _frame_host form of each.  One table: (call, defect, error code, lumahip_last_error's text).  Every row is one refused call at
64 x 32, profile 2, one frame -- a 16-pixel block fits four times in x and twice in y -- after which the output, the guard words behind
it and every input must be as they were.  A row with two defects ("a + b") states which of the two is reported: the block size comes
first, then the order of the family's plan; the host forms report null arguments, the block, the light level's scale, the staging's
findings and a word count below the map's, in this order.

The texts are the library's as it stood before the plans were put on one record of what a launch delivers (MeasureOut,
lumahip_internal.hpp); one row differs from then, MOM_DEV_ROW: the frame-fed moments map used to call its output map_dev there."""
import ctypes as C

import numpy as np
import pytest

from tests.support.device import Frames, L, Planes, ctx  # noqa: F401  (L is the module fixture)
from tests.support.host import CFG, ERR_ARG, ERR_STATE, GUARD, OUT_FILL, float_frames

pytestmark = pytest.mark.gpu

W, H, PROFILE, NF = 64, 32, 2, 1
ST = (128, 64, 64)                      # rows of 64 and 32 samples of two bytes
WORDS = {"frame": 12, "map": 4 * 2 * 12, "moments": 8 * 4 * 15, "light": 8}   # blocks of 16 (map) and of 8 (moments)
BLOCK = {"map": 16, "moments": 8}

# family -> the C parameters behind the context, in order; "block" is passed to the two maps only, "words" to their host forms only
ORDER = {
    "frames_dev": ("rgb", "frame_stride", "nframes", "w", "h", "sc", "profile", "planes", "stride", "pfs", "block", "out"),
    "frames_host": ("rgb", "w", "h", "sc", "profile", "planes", "stride", "block", "out", "words"),
    "trans_dev": ("src_planes", "src_stride", "src_pfs", "src_profile", "src_sc", "nframes", "w", "h", "planes", "stride", "pfs", "profile",
                  "sc", "block", "out"),
    "trans_host": ("src_planes", "src_stride", "src_profile", "src_sc", "w", "h", "planes", "stride", "profile", "sc", "block", "out", "words"),
    "p2p_dev": ("src_planes", "src_stride", "src_pfs", "nframes", "w", "h", "planes", "stride", "pfs", "profile", "block", "out"),
    "p2p_host": ("src_planes", "src_stride", "w", "h", "planes", "stride", "profile", "block", "out", "words"),
    "light_dev": ("rgb", "frame_stride", "nframes", "w", "h", "scale", "out"),
    "light_host": ("rgb", "w", "h", "scale", "out"),
    "plight_dev": ("planes", "stride", "pfs", "nframes", "w", "h", "profile", "sc", "scale", "out"),
    "plight_host": ("planes", "stride", "w", "h", "profile", "sc", "scale", "out"),
}
# the context a family's calls are accepted on: "q" has both quantizers, "bare" never had one
CTX = {"frames": "q", "trans": "q", "p2p": "bare", "light": "bare", "plight": "q"}


def call_of(symbol):
    """(family, kind, frames' form) of an entry point, from its name"""
    name = symbol[len("lumahip_"):]
    host = name.endswith("_frame_host")
    stem = name[:-len("_frame_host")] if host else name.split("_frames_device")[0]
    form = "" if host else name.split("_frames_device")[1]
    kind = "light" if stem.endswith("light_level") else "moments" if stem.endswith("moments_map") else "map" if stem.endswith("_map") else "frame"
    fam = ("plight" if stem == "planes_light_level" else "light" if stem == "light_level" else "trans" if stem.startswith("transcode_")
           else "p2p" if stem.startswith("planes_") else "frames")
    return fam + ("_host" if host else "_dev"), kind, form


class World:
    """the three contexts, one frame as floats and as halves, two plane sets, and the same in host memory"""

    def __init__(self, L):
        cfg = CFG["pq11_luv8"]
        self.ctx = {"q": ctx(L, cfg, src_cfg=cfg), "nosrc": ctx(L, cfg), "bare": ctx(L, None, quantizer=False)}
        fr = float_frames(np.random.default_rng(7), NF, W, H, halves=True)
        self.frames = {4: Frames(fr), 2: Frames(fr, dtype=np.float16)}
        self.a, self.b = (Planes(L, W, H, PROFILE, NF, strides=ST) for _ in range(2))
        self.rgb_host = np.ascontiguousarray(fr[0])
        self.rgb_was = self.rgb_host.copy()
        self.ha, self.hb = ([np.ascontiguousarray(x) for x in p.frame(p.host(), 0)] for p in (self.a, self.b))
        self.h_was = [x.copy() for x in self.ha + self.hb]

    def inputs_as_before(self):
        return (all(f.unchanged() for f in self.frames.values()) and self.a.unchanged() and self.b.unchanged()
                and np.array_equal(self.rgb_host, self.rgb_was) and all(np.array_equal(x, y) for x, y in zip(self.ha + self.hb, self.h_was)))


@pytest.fixture(scope="module")
def world(L):
    return World(L)


def accepted_args(wd, fam, form):
    """the arguments of a call the library accepts (block, out and words are the caller's to add)"""
    host = fam.endswith("_host")
    a = dict(w=W, h=H, sc=1.0, src_sc=1.0, scale=1.0, profile=PROFILE, src_profile=PROFILE, nframes=NF, ctx=CTX[fam.split("_")[0]])
    if host:
        a.update(rgb=wd.rgb_host.ctypes.data, src_planes=[p.ctypes.data for p in wd.ha], planes=[p.ctypes.data for p in wd.hb])
    else:
        fr = wd.frames[2 if form.endswith("f16") else 4]
        esz = 2 if form.endswith("f16") else 4
        a.update(rgb=[fr.ptr + k * fr.n * esz for k in range(3)] if "planar" in form else fr.ptr, esz=esz, frame_stride=fr.fs,
                 src_planes=list(wd.a.ptrs), planes=list(wd.b.ptrs), src_pfs=list(wd.a.pfs), pfs=list(wd.b.pfs))
    a.update(src_stride=list(ST), stride=list(ST))
    return a


def first_plane(a):
    return a["rgb"][0] if isinstance(a["rgb"], list) else a["rgb"]


def shifted(a, by):
    a["rgb"] = [p + by for p in a["rgb"]] if isinstance(a["rgb"], list) else a["rgb"] + by


# defect -> what it does to the arguments of an accepted call
DEFECTS = {
    "block 4": lambda a: a.update(block=4),
    "block 8": lambda a: a.update(block=8),
    "block 128": lambda a: a.update(block=128),
    "null frames": lambda a: a.update(rgb=[a["rgb"][0], None, a["rgb"][2]] if isinstance(a["rgb"], list) else None),
    "null planes": lambda a: a.update(planes=None),
    "null strides": lambda a: a.update(stride=None),
    "null frame strides": lambda a: a.update(pfs=None),
    "null source planes": lambda a: a.update(src_planes=None),
    "null plane 1": lambda a: a["planes"].__setitem__(1, None),
    "null source plane 2": lambda a: a["src_planes"].__setitem__(2, None),
    "no frames": lambda a: a.update(nframes=0),
    "odd width": lambda a: a.update(w=63),
    "zero height": lambda a: a.update(h=0),
    "profile 4": lambda a: a.update(profile=4),
    "source profile 4": lambda a: a.update(src_profile=4),
    "no quantizer": lambda a: a.update(ctx="bare"),
    "no source quantizer": lambda a: a.update(ctx="nosrc"),
    "short stride": lambda a: a["stride"].__setitem__(1, 16),
    "short source stride": lambda a: a["src_stride"].__setitem__(1, 16),
    "colour planes 8 bytes apart": lambda a: a["rgb"].__setitem__(1, a["rgb"][0] + 8),
    "frames off by one element": lambda a: shifted(a, a["esz"]),
    "scale 0": lambda a: a.update(scale=0.0),
    "scale inf": lambda a: a.update(scale=float("inf")),
    "null output": lambda a: a.update(out=lambda own: None),
    "output off by 4": lambda a: a.update(out=lambda own: own + 4),
    "output in the frames": lambda a: a.update(out=lambda own, p=first_plane(a): p + 64),
    "output in plane 0": lambda a: a.update(out=lambda own, p=a["planes"][0]: p + 64),
    "output in plane 2": lambda a: a.update(out=lambda own, p=a["planes"][2]: p + 8),
    "output in source plane 0": lambda a: a.update(out=lambda own, p=a["src_planes"][0]: p + 64),
    "output reaching into plane 1": lambda a: a.update(out=lambda own, p=a["planes"][1]: p - 40),
    "one word short": lambda a: a.update(words=a["words"] - 1),
}

NULL_ARG, NULL_PLANE_1 = "null argument", "null plane 1"
ODD = "Invalid frame size 63x32 (must be even, non-zero)"
PROFILE_4, SRC_PROFILE_4 = "profile must be 0..3 (got 4)", "source profile must be 0..3 (got 4)"
NO_Q = "quantizer not set (call lumahip_set_quantizer first)"
NO_SRC_Q = "source quantizer not set (call lumahip_set_source_quantizer first)"
SHORT_STRIDE = "plane 1: stride 16 < row bytes 64"
OUT_PTR, MAP_PTR, MOM_PTR = ("%s must be non-null and 8-byte aligned" % n for n in ("out_dev", "map_dev", "mom_dev"))
FRAMES_8, FRAMES_4 = ("colour planes must be %d-byte aligned and the frame stride even" % n for n in (8, 4))
SCALE_0, SCALE_INF = ("light level: scale must be finite and > 0 (got %s)" % v for v in ("0", "inf"))
MAP_BLOCK = "%s: block must be 16, 32 or 64 (got %d)"
MOM_BLOCK = "%s: block must be 8, 16, 32 or 64 (got %d)"

# the one row whose text changed with the record: (call, defect)
MOM_DEV_ROW = ("lumahip_moments_map_frames_device", "null output")

ROWS = [
    # ---- frame-fed, device forms: distortion_plan's order
    ("lumahip_distortion_map_frames_device", "block 4", ERR_ARG, MAP_BLOCK % ("distortion map", 4)),
    ("lumahip_distortion_map_frames_device_planar_f16", "block 8", ERR_ARG, MAP_BLOCK % ("distortion map", 8)),
    ("lumahip_moments_map_frames_device_planar", "block 4", ERR_ARG, MOM_BLOCK % ("moments map", 4)),
    ("lumahip_moments_map_frames_device_f16", "block 128", ERR_ARG, MOM_BLOCK % ("moments map", 128)),
    ("lumahip_distortion_frames_device", "null frames", ERR_ARG, NULL_ARG),
    ("lumahip_distortion_map_frames_device_planar", "null frames", ERR_ARG, NULL_ARG),
    ("lumahip_moments_map_frames_device_f16", "null frames", ERR_ARG, NULL_ARG),
    ("lumahip_distortion_frames_device_planar_f16", "null planes", ERR_ARG, NULL_ARG),
    ("lumahip_distortion_map_frames_device", "null strides", ERR_ARG, NULL_ARG),
    ("lumahip_moments_map_frames_device", "null frame strides", ERR_ARG, NULL_ARG),
    ("lumahip_distortion_frames_device", "no frames", ERR_ARG, NULL_ARG),
    ("lumahip_distortion_frames_device_planar", "null plane 1", ERR_ARG, NULL_PLANE_1),
    ("lumahip_moments_map_frames_device_planar_f16", "null plane 1", ERR_ARG, NULL_PLANE_1),
    ("lumahip_distortion_frames_device", "no quantizer", ERR_STATE, NO_Q),
    ("lumahip_distortion_map_frames_device_f16", "no quantizer", ERR_STATE, NO_Q),
    ("lumahip_distortion_frames_device_f16", "odd width", ERR_ARG, ODD),
    ("lumahip_distortion_map_frames_device", "odd width", ERR_ARG, ODD),
    ("lumahip_moments_map_frames_device_planar", "zero height", ERR_ARG, "Invalid frame size 64x0 (must be even, non-zero)"),
    ("lumahip_distortion_frames_device_planar", "profile 4", ERR_ARG, PROFILE_4),
    ("lumahip_moments_map_frames_device", "profile 4", ERR_ARG, PROFILE_4),
    ("lumahip_distortion_frames_device", "short stride", ERR_ARG, SHORT_STRIDE),
    ("lumahip_distortion_map_frames_device_planar_f16", "short stride", ERR_ARG, SHORT_STRIDE),
    ("lumahip_distortion_frames_device_planar", "colour planes 8 bytes apart", ERR_ARG,
     "colour planes 0 and 1 (2 floats apart, frame stride 6148): planes of different frames would overlap"),
    ("lumahip_distortion_frames_device", "null output", ERR_ARG, OUT_PTR),
    ("lumahip_distortion_frames_device_planar_f16", "output off by 4", ERR_ARG, OUT_PTR),
    ("lumahip_distortion_map_frames_device", "null output", ERR_ARG, MAP_PTR),
    ("lumahip_distortion_map_frames_device_f16", "output off by 4", ERR_ARG, MAP_PTR),
    MOM_DEV_ROW + (ERR_ARG, MOM_PTR),
    ("lumahip_distortion_frames_device", "frames off by one element", ERR_ARG, FRAMES_8),
    ("lumahip_distortion_map_frames_device_planar", "frames off by one element", ERR_ARG, FRAMES_8),
    ("lumahip_moments_map_frames_device_f16", "frames off by one element", ERR_ARG, FRAMES_4),
    ("lumahip_distortion_frames_device", "output in the frames", ERR_ARG, "out_dev overlaps colour plane 0 of the frames"),
    ("lumahip_distortion_map_frames_device_planar_f16", "output in the frames", ERR_ARG, "map_dev overlaps colour plane 0 of the frames"),
    ("lumahip_moments_map_frames_device", "output in the frames", ERR_ARG, "mom_dev overlaps colour plane 0 of the frames"),
    ("lumahip_distortion_frames_device_f16", "output in plane 2", ERR_ARG, "out_dev overlaps given plane 2"),
    ("lumahip_distortion_map_frames_device", "output reaching into plane 1", ERR_ARG, "map_dev overlaps given plane 1"),
    ("lumahip_moments_map_frames_device_planar", "output in plane 0", ERR_ARG, "mom_dev overlaps given plane 0"),
    ("lumahip_distortion_map_frames_device", "block 4 + odd width", ERR_ARG, MAP_BLOCK % ("distortion map", 4)),
    ("lumahip_moments_map_frames_device", "block 4 + no quantizer", ERR_ARG, MOM_BLOCK % ("moments map", 4)),
    ("lumahip_distortion_frames_device", "null plane 1 + output off by 4", ERR_ARG, NULL_PLANE_1),
    ("lumahip_distortion_frames_device", "null plane 1 + no quantizer", ERR_ARG, NULL_PLANE_1),
    ("lumahip_distortion_map_frames_device", "short stride + null output", ERR_ARG, SHORT_STRIDE),
    ("lumahip_distortion_frames_device", "output off by 4 + frames off by one element", ERR_ARG, OUT_PTR),
    # ---- frame-fed, host forms
    ("lumahip_distortion_frame_host", "null frames", ERR_ARG, NULL_ARG),
    ("lumahip_distortion_map_frame_host", "null planes", ERR_ARG, NULL_ARG),
    ("lumahip_moments_map_frame_host", "null strides", ERR_ARG, NULL_ARG),
    ("lumahip_distortion_frame_host", "null output", ERR_ARG, NULL_ARG),
    ("lumahip_distortion_map_frame_host", "block 8", ERR_ARG, MAP_BLOCK % ("distortion map", 8)),
    ("lumahip_moments_map_frame_host", "block 4", ERR_ARG, MOM_BLOCK % ("moments map", 4)),
    ("lumahip_distortion_frame_host", "no quantizer", ERR_STATE, NO_Q),
    ("lumahip_distortion_map_frame_host", "odd width", ERR_ARG, ODD),
    ("lumahip_moments_map_frame_host", "profile 4", ERR_ARG, PROFILE_4),
    ("lumahip_distortion_frame_host", "short stride", ERR_ARG, "plane 1: null or stride 16 < row bytes 64"),
    ("lumahip_distortion_map_frame_host", "null plane 1", ERR_ARG, "plane 1: null or stride 64 < row bytes 64"),
    ("lumahip_distortion_map_frame_host", "one word short", ERR_ARG, "distortion map: 95 words for a map of 96"),
    ("lumahip_moments_map_frame_host", "one word short", ERR_ARG, "moments map: 479 words for a map of 480"),
    ("lumahip_distortion_map_frame_host", "block 4 + one word short", ERR_ARG, MAP_BLOCK % ("distortion map", 4)),
    ("lumahip_moments_map_frame_host", "odd width + one word short", ERR_ARG, ODD),
    ("lumahip_moments_map_frame_host", "null output + block 4", ERR_ARG, NULL_ARG),
    # ---- plane-fed, device forms: transcode_plan's order
    ("lumahip_transcode_distortion_map_frames_device", "block 8", ERR_ARG, MAP_BLOCK % ("transcode distortion map", 8)),
    ("lumahip_transcode_moments_map_frames_device", "block 4", ERR_ARG, MOM_BLOCK % ("transcode moments map", 4)),
    ("lumahip_transcode_distortion_frames_device", "null source planes", ERR_ARG, NULL_ARG),
    ("lumahip_transcode_distortion_map_frames_device", "null frame strides", ERR_ARG, NULL_ARG),
    ("lumahip_transcode_moments_map_frames_device", "no frames", ERR_ARG, NULL_ARG),
    ("lumahip_transcode_distortion_frames_device", "null plane 1", ERR_ARG, NULL_PLANE_1),
    ("lumahip_transcode_moments_map_frames_device", "null source plane 2", ERR_ARG, "null plane 2"),
    ("lumahip_transcode_distortion_frames_device", "no quantizer", ERR_STATE, NO_Q),
    ("lumahip_transcode_distortion_map_frames_device", "odd width", ERR_ARG, ODD),
    ("lumahip_transcode_moments_map_frames_device", "profile 4", ERR_ARG, PROFILE_4),
    ("lumahip_transcode_distortion_frames_device", "source profile 4", ERR_ARG, SRC_PROFILE_4),
    ("lumahip_transcode_distortion_map_frames_device", "no source quantizer", ERR_STATE, NO_SRC_Q),
    ("lumahip_transcode_distortion_frames_device", "short source stride", ERR_ARG, SHORT_STRIDE),
    ("lumahip_transcode_moments_map_frames_device", "short stride", ERR_ARG, SHORT_STRIDE),
    ("lumahip_transcode_distortion_frames_device", "null output", ERR_ARG, OUT_PTR),
    ("lumahip_transcode_distortion_map_frames_device", "output off by 4", ERR_ARG, MAP_PTR),
    ("lumahip_transcode_moments_map_frames_device", "null output", ERR_ARG, MOM_PTR),
    ("lumahip_transcode_distortion_frames_device", "output in source plane 0", ERR_ARG, "out_dev overlaps source plane 0"),
    ("lumahip_transcode_distortion_map_frames_device", "output in plane 2", ERR_ARG, "map_dev overlaps given plane 2"),
    ("lumahip_transcode_moments_map_frames_device", "output in plane 0", ERR_ARG, "mom_dev overlaps given plane 0"),
    ("lumahip_transcode_moments_map_frames_device", "block 4 + no source quantizer", ERR_ARG, MOM_BLOCK % ("transcode moments map", 4)),
    ("lumahip_transcode_distortion_frames_device", "source profile 4 + no source quantizer", ERR_ARG, SRC_PROFILE_4),
    ("lumahip_transcode_distortion_map_frames_device", "no source quantizer + null output", ERR_STATE, NO_SRC_Q),
    # ---- plane-fed, host forms
    ("lumahip_transcode_distortion_frame_host", "null source planes", ERR_ARG, NULL_ARG),
    ("lumahip_transcode_moments_map_frame_host", "null output", ERR_ARG, NULL_ARG),
    ("lumahip_transcode_distortion_map_frame_host", "block 4", ERR_ARG, MAP_BLOCK % ("transcode distortion map", 4)),
    ("lumahip_transcode_moments_map_frame_host", "block 128", ERR_ARG, MOM_BLOCK % ("transcode moments map", 128)),
    ("lumahip_transcode_distortion_frame_host", "no quantizer", ERR_STATE, NO_Q),
    ("lumahip_transcode_distortion_frame_host", "source profile 4", ERR_ARG, SRC_PROFILE_4),
    ("lumahip_transcode_distortion_map_frame_host", "no source quantizer", ERR_STATE, NO_SRC_Q),
    ("lumahip_transcode_distortion_frame_host", "short source stride", ERR_ARG, "source plane 1: null or stride 16 < row bytes 64"),
    ("lumahip_transcode_moments_map_frame_host", "null plane 1", ERR_ARG, "given plane 1: null or stride 64 < row bytes 64"),
    ("lumahip_transcode_distortion_map_frame_host", "one word short", ERR_ARG, "transcode distortion map: 95 words for a map of 96"),
    ("lumahip_transcode_moments_map_frame_host", "one word short", ERR_ARG, "transcode moments map: 479 words for a map of 480"),
    ("lumahip_transcode_moments_map_frame_host", "block 4 + one word short", ERR_ARG, MOM_BLOCK % ("transcode moments map", 4)),
    # ---- plane-to-plane, device forms: planes_plan's order
    ("lumahip_planes_distortion_map_frames_device", "block 8", ERR_ARG, MAP_BLOCK % ("planes distortion map", 8)),
    ("lumahip_planes_moments_map_frames_device", "block 4", ERR_ARG, MOM_BLOCK % ("planes moments map", 4)),
    ("lumahip_planes_distortion_frames_device", "null source planes", ERR_ARG, NULL_ARG),
    ("lumahip_planes_distortion_map_frames_device", "no frames", ERR_ARG, NULL_ARG),
    ("lumahip_planes_moments_map_frames_device", "null plane 1", ERR_ARG, NULL_PLANE_1),
    ("lumahip_planes_distortion_frames_device", "odd width", ERR_ARG, ODD),
    ("lumahip_planes_distortion_map_frames_device", "profile 4", ERR_ARG, PROFILE_4),
    ("lumahip_planes_moments_map_frames_device", "short source stride", ERR_ARG, SHORT_STRIDE),
    ("lumahip_planes_distortion_frames_device", "output off by 4", ERR_ARG, OUT_PTR),
    ("lumahip_planes_distortion_map_frames_device", "null output", ERR_ARG, MAP_PTR),
    ("lumahip_planes_moments_map_frames_device", "output off by 4", ERR_ARG, MOM_PTR),
    ("lumahip_planes_distortion_frames_device", "output in source plane 0", ERR_ARG, "out_dev overlaps plane 0 of set A"),
    ("lumahip_planes_distortion_map_frames_device", "output in plane 2", ERR_ARG, "map_dev overlaps plane 2 of set B"),
    ("lumahip_planes_moments_map_frames_device", "output in plane 0", ERR_ARG, "mom_dev overlaps plane 0 of set B"),
    ("lumahip_planes_distortion_map_frames_device", "block 4 + odd width", ERR_ARG, MAP_BLOCK % ("planes distortion map", 4)),
    ("lumahip_planes_distortion_frames_device", "null plane 1 + output off by 4", ERR_ARG, NULL_PLANE_1),
    ("lumahip_planes_moments_map_frames_device", "profile 4 + null output", ERR_ARG, PROFILE_4),
    # ---- plane-to-plane, host forms
    ("lumahip_planes_distortion_frame_host", "null strides", ERR_ARG, NULL_ARG),
    ("lumahip_planes_distortion_map_frame_host", "block 8", ERR_ARG, MAP_BLOCK % ("planes distortion map", 8)),
    ("lumahip_planes_moments_map_frame_host", "block 4", ERR_ARG, MOM_BLOCK % ("planes moments map", 4)),
    ("lumahip_planes_distortion_frame_host", "odd width", ERR_ARG, ODD),
    ("lumahip_planes_distortion_map_frame_host", "profile 4", ERR_ARG, PROFILE_4),
    ("lumahip_planes_distortion_frame_host", "short source stride", ERR_ARG, "set A plane 1: null or stride 16 < row bytes 64"),
    ("lumahip_planes_moments_map_frame_host", "null plane 1", ERR_ARG, "set B plane 1: null or stride 64 < row bytes 64"),
    ("lumahip_planes_distortion_map_frame_host", "one word short", ERR_ARG, "planes distortion map: 95 words for a map of 96"),
    ("lumahip_planes_moments_map_frame_host", "one word short", ERR_ARG, "planes moments map: 479 words for a map of 480"),
    ("lumahip_planes_distortion_map_frame_host", "block 4 + one word short", ERR_ARG, MAP_BLOCK % ("planes distortion map", 4)),
    ("lumahip_planes_moments_map_frame_host", "profile 4 + one word short", ERR_ARG, PROFILE_4),
    # ---- light level of frames: light_plan's order
    ("lumahip_light_level_frames_device", "null frames", ERR_ARG, NULL_ARG),
    ("lumahip_light_level_frames_device_planar_f16", "null frames", ERR_ARG, NULL_ARG),
    ("lumahip_light_level_frames_device_f16", "no frames", ERR_ARG, "light level: nframes must be at least 1"),
    ("lumahip_light_level_frames_device_planar", "odd width", ERR_ARG, ODD),
    ("lumahip_light_level_frames_device", "scale 0", ERR_ARG, SCALE_0),
    ("lumahip_light_level_frames_device_planar_f16", "scale inf", ERR_ARG, SCALE_INF),
    ("lumahip_light_level_frames_device", "null output", ERR_ARG, OUT_PTR),
    ("lumahip_light_level_frames_device_f16", "output off by 4", ERR_ARG, OUT_PTR),
    ("lumahip_light_level_frames_device_planar", "frames off by one element", ERR_ARG, FRAMES_8),
    ("lumahip_light_level_frames_device_f16", "frames off by one element", ERR_ARG, FRAMES_4),
    ("lumahip_light_level_frames_device", "output in the frames", ERR_ARG, "out_dev overlaps colour plane 0 of the frames"),
    ("lumahip_light_level_frames_device", "odd width + scale 0", ERR_ARG, ODD),
    ("lumahip_light_level_frames_device", "scale 0 + null output", ERR_ARG, SCALE_0),
    ("lumahip_light_level_frame_host", "null frames", ERR_ARG, NULL_ARG),
    ("lumahip_light_level_frame_host", "null output", ERR_ARG, NULL_ARG),
    ("lumahip_light_level_frame_host", "odd width", ERR_ARG, ODD),
    ("lumahip_light_level_frame_host", "scale 0", ERR_ARG, SCALE_0),
    ("lumahip_light_level_frame_host", "odd width + scale 0", ERR_ARG, ODD),
    # ---- light level of code planes
    ("lumahip_planes_light_level_frames_device", "null planes", ERR_ARG, NULL_ARG),
    ("lumahip_planes_light_level_frames_device", "null plane 1", ERR_ARG, NULL_PLANE_1),
    ("lumahip_planes_light_level_frames_device", "no frames", ERR_ARG, "light level: nframes must be at least 1"),
    ("lumahip_planes_light_level_frames_device", "odd width", ERR_ARG, ODD),
    ("lumahip_planes_light_level_frames_device", "scale 0", ERR_ARG, SCALE_0),
    ("lumahip_planes_light_level_frames_device", "output off by 4", ERR_ARG, OUT_PTR),
    ("lumahip_planes_light_level_frames_device", "profile 4", ERR_ARG, PROFILE_4),
    ("lumahip_planes_light_level_frames_device", "no quantizer", ERR_STATE, NO_Q),
    ("lumahip_planes_light_level_frames_device", "short stride", ERR_ARG, SHORT_STRIDE),
    ("lumahip_planes_light_level_frames_device", "output in plane 2", ERR_ARG, "out_dev overlaps plane 2"),
    ("lumahip_planes_light_level_frames_device", "profile 4 + scale 0", ERR_ARG, SCALE_0),
    ("lumahip_planes_light_level_frames_device", "no quantizer + null output", ERR_ARG, OUT_PTR),
    ("lumahip_planes_light_level_frame_host", "null planes", ERR_ARG, NULL_ARG),
    ("lumahip_planes_light_level_frame_host", "scale 0", ERR_ARG, SCALE_0),
    ("lumahip_planes_light_level_frame_host", "no quantizer", ERR_STATE, NO_Q),
    ("lumahip_planes_light_level_frame_host", "odd width", ERR_ARG, ODD),
    ("lumahip_planes_light_level_frame_host", "profile 4", ERR_ARG, PROFILE_4),
    ("lumahip_planes_light_level_frame_host", "short stride", ERR_ARG, "plane 1: null or stride 16 < row bytes 64"),
    ("lumahip_planes_light_level_frame_host", "odd width + scale 0", ERR_ARG, SCALE_0),
]


def c_value(name, v):
    """a Python value as the C parameter `name` takes it"""
    if isinstance(v, list):
        elem = C.c_void_p if name in ("rgb", "planes", "src_planes") else C.c_size_t if name.endswith("pfs") else C.c_int
        return (elem * 3)(*v)
    return v


@pytest.mark.parametrize("symbol, defect, code, text", ROWS, ids=["%s-%s" % (r[0][len("lumahip_"):], r[1].replace(" ", "_")) for r in ROWS])
def test_refused(L, world, symbol, defect, code, text):
    import torch
    fam, kind, form = call_of(symbol)
    host = fam.endswith("_host")
    a = accepted_args(world, fam, form)
    a.update(block=BLOCK.get(kind), words=WORDS[kind], out=lambda own: own)
    for d in defect.split(" + "):
        DEFECTS[d](a)
    if host:
        buf = np.full(WORDS[kind] + GUARD, OUT_FILL, dtype=np.int64)
        own = buf.ctypes.data
    else:
        buf = torch.full((WORDS[kind] + GUARD,), OUT_FILL, dtype=torch.int64, device=world.a.t[0].device)
        own = buf.data_ptr()
    a["out"] = a["out"](own)
    names = [n for n in ORDER[fam] if (n != "block" or kind in BLOCK) and (n != "words" or kind in BLOCK)]
    c = world.ctx[a["ctx"]]
    rc = getattr(c.L, symbol)(c.h, *[c_value(n, a[n]) for n in names])
    assert (rc, c.L.lumahip_last_error(c.h).decode()) == (code, text)
    if not host:
        torch.cuda.synchronize()
        buf = buf.cpu().numpy()
    assert np.all(buf == OUT_FILL), "a refused call wrote to its output or to the guard words behind it"
    assert world.inputs_as_before(), "a refused call changed an input"
