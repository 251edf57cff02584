#!/usr/bin/env python3
"""tools/bench/transcode_distortion_map.py [--rounds R] [--min-s S] [--out FILE] -- the transcode distortion map launch against what
it replaces and against the per-frame transcode distortion launch.

Workloads: PQ-11 Lu'v' planes -> LOG-12 Lu'v' and -> the HDR10 Y'CbCr recipe (PQ-10, 10-bit colour, sc 20); profile 2 on both
sides, 8 frames of 3840x2160 per launch, ordered launches on one stream, plain allocations, one process on one box, four distinct
batches; blocks of 16 and of 64 luma pixels.  The given planes are the source planes' own transcode under a target preScaling 2 %
off, as in tools/bench/transcode_distortion.py.  Legs, interleaved round by round:
  `map`      = lumahip_transcode_distortion_map_frames_device;
  `replaced` = lumahip_transcode_frames_device into scratch planes, then the torch reduction per block that yields the same words
               (tools/bench/distortion_map.py torch_block_reduction);
  `frame`    = lumahip_transcode_distortion_frames_device on the same inputs: twelve words per frame, one memset and global atomics
               (its code does not change with the map's, so this leg is also the yardstick between two builds on one box).
Per leg and round: hipEvent time of back-to-back launches, at least --min-s seconds of device time; the median round is reported.
The integers of `map` and `replaced` are compared once before anything is timed, and the map folded per frame against `frame`.
-> profiles/transcode_distortion_map.jsonl: every run APPENDS one JSON line with, per workload and block size, ms and Mpixel/s of
each leg, map over replaced (the bar: >= 1), map's time over frame's (recorded, not a bar) and the spread of the rounds."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import lumahdrv_amd as L  # noqa: E402
from lumahdrv_amd import capi  # noqa: E402
from tools.bench.distortion_map import BLOCKS, torch_block_reduction  # noqa: E402
from tools.bench.transcode_distortion import SRC, TARGETS  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--min-s", type=float, default=1.0, help="device time per leg and round")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transcode_distortion_map.jsonl"), help="'' = print only")
    ap.add_argument("--only", default="", help="one target, e.g. pq10_ycbcr10 (for rocprofv3 captures)")
    ap.add_argument("--leg", default="", help="map, replaced or frame: that leg only, one round, nothing written")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    w, h, B, nb, profile = 3840, 2160, a.frames, 4, 2
    n, n3 = w * h, 3 * w * h
    _, hs, st, _ = L.plane_geometry(w, h, profile)
    psz = [hs[p] * st[p] for p in range(3)]
    dims = [(hs[p], st[p] // 2) for p in range(3)]
    assert dims == [(h, w), (h // 2, w // 2), (h // 2, w // 2)], "planes without row padding at this size"
    s = torch.cuda.current_stream()
    scfg, src_sc = SRC

    def at(t, b):
        return [t[p].data_ptr() + b * B * psz[p] for p in range(3)]

    # the archive: nb batches of B frames as PQ-11 Lu'v' planes (the float frames exist only to make them)
    src = [torch.zeros(nb * B * psz[p], dtype=torch.uint8, device=dev) for p in range(3)]
    cs = L.Context(0)
    cs.set_stream(s.cuda_stream)
    cs.set_quantizer(*scfg, L.build_lut(scfg[0], scfg[1], scfg[4], scfg[5]))
    f32 = torch.empty(B * n3, dtype=torch.float32, device=dev)
    for b in range(nb):
        cs.synth_frames_device(f32.data_ptr(), n3, B, w, h)
        f32 *= 1.0 + 0.25 * b   # (distinct batches)
        cs.encode_frames_device(f32.data_ptr(), n3, B, w, h, src_sc, profile, at(src, b), st, psz)
    torch.cuda.synchronize()
    cs.close()
    del f32
    torch.cuda.empty_cache()

    rows = []
    for name, (cfg, dst_sc) in TARGETS.items():
        if a.only and a.only != name:
            continue
        tag = "pq11_luv8->" + name
        c = L.Context(0)
        c.set_stream(s.cuda_stream)
        c.set_quantizer(*cfg, L.build_lut(cfg[0], cfg[1], cfg[4], cfg[5]))
        c.set_source_quantizer(*scfg, L.build_lut(scfg[0], scfg[1], scfg[4], scfg[5]))
        given = [torch.zeros(nb * B * psz[p], dtype=torch.uint8, device=dev) for p in range(3)]
        scratch = [torch.zeros(B * psz[p], dtype=torch.uint8, device=dev) for p in range(3)]
        out_f = torch.zeros(nb, B, 3, 4, dtype=torch.int64, device=dev)
        for b in range(nb):
            c.transcode_frames_device(at(src, b), st, psz, profile, src_sc, B, w, h, at(given, b), st, psz, profile, dst_sc * 1.02)

        for block in BLOCKS:
            nbx, nby = capi.distortion_map_dims(w, h, block)
            out_m = torch.full((nb, B, nby, nbx, 3, 4), -1, dtype=torch.int64, device=dev)   # (the launch writes every word)
            out_r = torch.zeros(nb, B, nby, nbx, 3, 4, dtype=torch.int64, device=dev)

            def launch(leg, b):
                if leg == "map":
                    c.transcode_distortion_map_frames_device(at(src, b), st, psz, profile, src_sc, B, w, h, at(given, b), st, psz, profile,
                                                             dst_sc, block, out_m[b].data_ptr())
                elif leg == "frame":
                    c.transcode_distortion_frames_device(at(src, b), st, psz, profile, src_sc, B, w, h, at(given, b), st, psz, profile,
                                                         dst_sc, out_f[b].data_ptr())
                else:
                    c.transcode_frames_device(at(src, b), st, psz, profile, src_sc, B, w, h, [t.data_ptr() for t in scratch], st, psz,
                                              profile, dst_sc)
                    torch_block_reduction(scratch, [given[p][b * B * psz[p]:(b + 1) * B * psz[p]] for p in range(3)], B, dims, block, out_r[b])

            for b in range(nb):   # the methods compute the same integers
                for leg in ("map", "replaced", "frame"):
                    launch(leg, b)
            torch.cuda.synchronize()
            if not torch.equal(out_m, out_r):
                raise SystemExit("%s, block %d: the map launch and the replaced method disagree" % (tag, block))
            fold = out_m.sum((2, 3))
            fold[..., 2] = out_m[..., 2].amax((2, 3))
            if not torch.equal(fold, out_f):
                raise SystemExit("%s, block %d: the map does not fold to the per-frame words" % (tag, block))
            differing = float(out_f[..., 3].sum()) / (nb * B * 1.5 * n)

            def timed(leg, iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                for i in range(iters):
                    launch(leg, i % nb)
                e1.record(s)
                e1.synchronize()
                return e0.elapsed_time(e1) / iters

            legs = [a.leg] if a.leg else ["map", "replaced", "frame"]
            iters = {}
            for leg in legs:   # warm-up, and how many launches make --min-s of device time
                timed(leg, 4)
                iters[leg] = max(4, int(a.min_s * 1e3 / timed(leg, 8)) + 1)
            res = {leg: [] for leg in legs}
            for r in range(1 if a.leg else a.rounds):
                for leg in (legs if r % 2 == 0 else legs[::-1]):
                    res[leg].append(timed(leg, iters[leg]))
            if a.leg:
                print("%s  block %d  %s: %.4f ms per launch" % (tag, block, a.leg, res[a.leg][0]))
            else:
                med = {leg: sorted(v)[len(v) // 2] for leg, v in res.items()}
                mpx = {leg: B * n / (med[leg] * 1e-3) / 1e6 for leg in legs}
                rows.append(dict(workload=tag, block=block, frames_per_launch=B, w=w, h=h, profile=profile, src_sc=src_sc, dst_sc=dst_sc,
                                 samples_differing=round(differing, 3), ms={leg: round(med[leg], 4) for leg in legs},
                                 mpixel_s={leg: round(mpx[leg], 1) for leg in legs}, map_over_replaced=round(mpx["map"] / mpx["replaced"], 3),
                                 map_ms_over_frame_ms=round(med["map"] / med["frame"], 3),
                                 spread={leg: round(max(v) / min(v) - 1, 4) for leg, v in res.items()}, launches_per_round=iters))
            del out_m, out_r
        c.close()
        del given, scratch, out_f
        torch.cuda.empty_cache()
    for r in rows:
        print("%-26s block %2d: map %8.4f ms | replaced %8.4f ms | per-frame distortion %8.4f ms | map x%.3f of replaced | map / frame %.3f | "
              "spread %s" % (r["workload"], r["block"], r["ms"]["map"], r["ms"]["replaced"], r["ms"]["frame"], r["map_over_replaced"],
                             r["map_ms_over_frame_ms"], r["spread"]))
    if a.out and rows:
        line = dict(rounds=a.rounds, min_s=a.min_s, kernel_source_sha=capi.kernel_source_sha(), device=torch.cuda.get_device_name(0),
                    library=os.path.basename(os.path.dirname(capi.library_path())), workloads=rows)
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")
    if rows and any(r["map_over_replaced"] < 1.0 for r in rows):
        raise SystemExit("the map launch is slower than the method it replaces")


if __name__ == "__main__":
    main()
