#!/usr/bin/env python3
"""tools/bench/planes_measure.py [--rounds R] [--min-s S] [--out FILE] [--sweep] -- the plane-to-plane measuring launches
(include/lumahip_compare.h) against what they replace and against the frame-fed launches that deliver the same words.

Workloads: profile 2 (16-bit 4:2:0, 6 B/pixel read) and profile 0 (8-bit 4:2:0, 3 B/pixel); 8 frames of 3840x2160 per launch, ordered
launches on one stream, plain allocations, one process on one box, four distinct batches.  Set A is the PQ-11 Lu'v' encode of the
tool's float frames, set B that encode at a preScaling 2 % off, as the other tools make their given planes.  Legs, interleaved round
by round, each as (per-frame words, distortion map at 16 and 64, moments map at 8 and 64):
  `planes`   = lumahip_planes_distortion_frames_device, lumahip_planes_distortion_map_frames_device, lumahip_planes_moments_map_frames_device
               on A and B;
  `replaced` = the torch reduction of the two plane sets to the same words: the torch halves of tools/bench/distortion.py,
               distortion_map.py and moments_map.py, imported.  They read 16-bit planes, so at profile 0 the replaced method first widens
               both sets to 16 bits (one torch op per plane), which is part of what it costs;
  `frames`   = lumahip_distortion_frames_device, lumahip_distortion_map_frames_device and lumahip_moments_map_frames_device on the float
               frames with B as the given planes: the launches that delivered these words before (15 B/pixel and a whole encode).
Per leg and round: hipEvent time of back-to-back launches, at least --min-s seconds of device time; the median round is reported.
Once before anything is timed: `planes` equals `replaced` and `frames`, word for word.
--sweep: additionally lumahip_tune("blocks_per_cu") over {3, 5, 8} on the `planes` legs, the values interleaved round by round, the
median of the rounds per value (a quarter of --min-s each); goes into the line.
-> profiles/planes_measure.jsonl: every run APPENDS one JSON line with, per workload, ms per launch of each leg, the ratios, the
fraction of 8 TB/s at 6 / 3 B/pixel (+ 96 or 120 B per block written) and the spread of the rounds.
Two gates, on the medians with the larger of the two legs' round spread as margin; the exit status is 1 below either:
  1. `planes` is no slower than `replaced`;   2. `planes` is no slower than `frames` on the same words.
A finding, not a gate: the traffic ratio of `planes` to `frames` is 0.4; the line records whether the profile-2 per-frame leg takes
more than 0.5 of `frames`' time (--leg planes:frame:0 runs that leg alone for a counters capture)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
from distortion import torch_reduction  # noqa: E402
from distortion_map import torch_block_reduction  # noqa: E402
from moments_map import torch_block_moments  # noqa: E402

import lumahdrv_amd as L  # noqa: E402
from lumahdrv_amd import capi  # noqa: E402

HBM = 8e12
CFG, SC = (L.PTF_PQ, 11, L.CS_LUV, 8, 1e4, 0.005), 1.0
PROFILES = (2, 0)
WHATS = [("frame", 0), ("map", 16), ("map", 64), ("moments", 8), ("moments", 64)]
METHODS = ("planes", "replaced", "frames")
SWEEP = (3, 5, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--min-s", type=float, default=1.0, help="device time per leg and round")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "planes_measure.jsonl"), help="'' = print only")
    ap.add_argument("--only", default="", help="one workload: p2 or p0")
    ap.add_argument("--leg", default="", help="method:what:block, e.g. planes:frame:0 or frames:moments:64: that leg only, one round, nothing written")
    ap.add_argument("--sweep", action="store_true", help="+ blocks_per_cu over {3, 5, 8} on the planes legs")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    w, h, B, nb = 3840, 2160, a.frames, 4
    n, n3 = w * h, 3 * w * h
    s = torch.cuda.current_stream()
    c = L.Context(0)
    c.set_stream(s.cuda_stream)
    c.set_quantizer(*CFG, L.build_lut(CFG[0], CFG[1], CFG[4], CFG[5]))
    bare = L.Context(0)                      # the plane-to-plane calls run on a context without a quantizer
    bare.set_stream(s.cuda_stream)
    f32 = torch.empty(nb * B * n3, dtype=torch.float32, device=dev)
    c.synth_frames_device(f32.data_ptr(), n3, nb * B, w, h)
    rows = []
    for profile in PROFILES:
        tag = "p%d" % profile
        if a.only and a.only != tag:
            continue
        bps = 2 if profile > 1 else 1
        _, hs, st, _ = L.plane_geometry(w, h, profile)
        psz = [hs[p] * st[p] for p in range(3)]
        dims = [(hs[p], st[p] // bps) for p in range(3)]
        assert dims == [(h, w), (h // 2, w // 2), (h // 2, w // 2)], "planes without row padding at this size"
        A = [torch.zeros(nb * B * psz[p], dtype=torch.uint8, device=dev) for p in range(3)]
        Bs = [torch.zeros(nb * B * psz[p], dtype=torch.uint8, device=dev) for p in range(3)]

        def fr(b):
            return f32.data_ptr() + b * B * n3 * 4

        def at(t, b):
            return [t[p].data_ptr() + b * B * psz[p] for p in range(3)]

        def batch(t, b):
            """batch b of a plane set as the torch halves take it: 16-bit samples behind uint8"""
            v = [t[p][b * B * psz[p]:(b + 1) * B * psz[p]] for p in range(3)]
            return v if bps == 2 else [x.to(torch.int16).view(torch.uint8) for x in v]

        for b in range(nb):
            c.encode_frames_device(fr(b), n3, B, w, h, SC, profile, at(A, b), st, psz)
            c.encode_frames_device(fr(b), n3, B, w, h, SC * 1.02, profile, at(Bs, b), st, psz)

        out = {}
        for m in METHODS:
            for what, block in WHATS:   # (the launches write every word of theirs, or zero them first)
                if what == "frame":
                    shape = (nb, B, 3, 4)
                else:
                    nbx, nby = capi.moments_map_dims(w, h, block)
                    shape = (nb, B, nby, nbx, 3, 4 if what == "map" else 5)
                out[m, what, block] = torch.full(shape, -1, dtype=torch.int64, device=dev)

        def launch(m, what, block, b):
            o = out[m, what, block][b]
            if m == "planes":
                two = (at(A, b), st, psz, B, w, h, at(Bs, b), st, psz, profile)
                if what == "frame":
                    bare.planes_distortion_frames_device(*two, o.data_ptr())
                elif what == "map":
                    bare.planes_distortion_map_frames_device(*two, block, o.data_ptr())
                else:
                    bare.planes_moments_map_frames_device(*two, block, o.data_ptr())
            elif m == "frames":
                fed = (fr(b), n3, B, w, h, SC, profile, at(Bs, b), st, psz)
                if what == "frame":
                    c.distortion_frames_device(*fed, o.data_ptr())
                elif what == "map":
                    c.distortion_map_frames_device(*fed, block, o.data_ptr())
                else:
                    c.moments_map_frames_device(*fed, block, o.data_ptr())
            else:
                e, g = batch(A, b), batch(Bs, b)
                if what == "frame":
                    torch_reduction(e, g, B, o)
                elif what == "map":
                    torch_block_reduction(e, g, B, dims, block, o)
                else:
                    torch_block_moments(e, g, B, dims, block, o)

        legs = [(m,) + wb for m in METHODS for wb in WHATS]
        for b in range(nb):   # the methods compute the same integers
            for leg in legs:
                launch(*leg, b)
        torch.cuda.synchronize()
        for what, block in WHATS:
            for m in ("replaced", "frames"):
                if not torch.equal(out["planes", what, block], out[m, what, block]):
                    raise SystemExit("%s, %s at block %d: `planes` and `%s` disagree" % (tag, what, block, m))
            if not (out["planes", what, block] != 0).any():
                raise SystemExit("%s, %s at block %d: all zeros" % (tag, what, block))

        def timed(leg, iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for i in range(iters):
                launch(*leg, i % nb)
            e1.record(s)
            e1.synchronize()
            return e0.elapsed_time(e1) / iters

        key = "%s_%s_%d".__mod__
        if a.leg:
            legs = [lg for lg in legs if a.leg == "%s:%s:%d" % lg]
            if not legs:
                raise SystemExit("--leg: method:what:block with method in %s and what:block in %s" % (METHODS, WHATS))
        iters = {}
        for lg in legs:   # warm-up, and how many launches make --min-s of device time
            timed(lg, 4)
            iters[lg] = max(4, int(a.min_s * 1e3 / timed(lg, 8)) + 1)
        res = {lg: [] for lg in legs}
        for r in range(1 if a.leg else a.rounds):
            for lg in (legs if r % 2 == 0 else legs[::-1]):
                res[lg].append(timed(lg, iters[lg]))
        if a.leg:
            print("%s  %s: %.4f ms per launch" % (tag, a.leg, res[legs[0]][0]))
            continue
        med = {lg: sorted(v)[len(v) // 2] for lg, v in res.items()}
        spread = {lg: max(v) / min(v) - 1 for lg, v in res.items()}

        def nbytes(what, block):
            if what == "frame":
                return B * (n * 3 * bps + 96)
            nbx, nby = capi.moments_map_dims(w, h, block)
            return B * (n * 3 * bps + nbx * nby * (96 if what == "map" else 120))

        gates = {}
        for other in ("replaced", "frames"):
            for wb in WHATS:
                p, o = ("planes",) + wb, (other,) + wb
                gates[key(o)] = bool(med[p] <= med[o] * (1 + max(spread[p], spread[o])))
        row = dict(workload=tag, frames_per_launch=B, w=w, h=h, profile=profile, bytes_per_pixel=3 * bps,
                   ms={key(lg): round(med[lg], 4) for lg in legs},
                   replaced_over_planes={"%s_%d" % wb: round(med[("replaced",) + wb] / med[("planes",) + wb], 3) for wb in WHATS},
                   planes_over_frames={"%s_%d" % wb: round(med[("planes",) + wb] / med[("frames",) + wb], 3) for wb in WHATS},
                   planes_fraction_of_8TBs={"%s_%d" % wb: round(nbytes(*wb) / (med[("planes",) + wb] * 1e-3) / HBM, 3) for wb in WHATS},
                   spread={key(lg): round(spread[lg], 4) for lg in legs},
                   launches_per_round={key(lg): iters[lg] for lg in legs},
                   planes_no_slower_than=gates)
        if profile == 2:
            row["per_frame_leg_above_half_of_frames"] = bool(med["planes", "frame", 0] > 0.5 * med["frames", "frame", 0])
        if a.sweep:
            plegs = [("planes",) + wb for wb in WHATS]
            sw = {(v, lg): [] for v in SWEEP for lg in plegs}
            for r in range(a.rounds):
                for v in (SWEEP if r % 2 == 0 else SWEEP[::-1]):
                    bare.tune("blocks_per_cu", v)
                    for lg in plegs:
                        sw[v, lg].append(timed(lg, max(4, iters[lg] // 4)))
            bare.tune("blocks_per_cu", 0)
            row["blocks_per_cu_sweep_ms"] = {"%s_%d" % lg[1:]: {str(v): round(sorted(sw[v, lg])[len(sw[v, lg]) // 2], 4) for v in SWEEP}
                                             for lg in plegs}
            row["blocks_per_cu_sweep_spread"] = {"%s_%d" % lg[1:]: {str(v): round(max(sw[v, lg]) / min(sw[v, lg]) - 1, 4) for v in SWEEP}
                                                 for lg in plegs}
        rows.append(row)
        del A, Bs, out
        torch.cuda.empty_cache()
    for r in rows:
        for wb in WHATS:
            k = "%s_%d" % wb
            print("%s %-10s planes %8.4f ms (%.3f of 8 TB/s) | replaced %9.4f ms (x%.3f) | frames %8.4f ms (planes / frames %.3f)" %
                  (r["workload"], k, r["ms"]["planes_" + k], r["planes_fraction_of_8TBs"][k], r["ms"]["replaced_" + k],
                   r["replaced_over_planes"][k], r["ms"]["frames_" + k], r["planes_over_frames"][k]))
        if "blocks_per_cu_sweep_ms" in r:
            print("%s blocks_per_cu sweep (ms): %s" % (r["workload"], json.dumps(r["blocks_per_cu_sweep_ms"])))
    if a.out and rows:
        line = dict(rounds=a.rounds, min_s=a.min_s, kernel_source_sha=capi.kernel_source_sha(), device=torch.cuda.get_device_name(0),
                    library=os.path.basename(os.path.dirname(capi.library_path())), workloads=rows)
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")
    bad = [(r["workload"], k) for r in rows for k, ok in r["planes_no_slower_than"].items() if not ok]
    if bad:
        print("gates failed: %s" % bad)
        raise SystemExit(1)


if __name__ == "__main__":
    main()
