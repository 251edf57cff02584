#!/usr/bin/env python3
"""tools/bench/distortion_map.py [--rounds R] [--min-s S] [--out FILE] -- the distortion map launch against what it replaces and
against the per-frame distortion launch.

Workloads: PQ-11 Lu'v' from float frames, PQ-11 Lu'v' from binary16 frames, the HDR10 Y'CbCr recipe (PQ-10, 10-bit colour, sc 20)
from binary16 frames; profile 2, 8 frames of 3840x2160 per launch, ordered launches on one stream, plain allocations, one process
on one box, four distinct batches; blocks of 16 and of 64 luma pixels.  The given planes are the frames' own planes under a
preScaling 2 % off, as in tools/bench/distortion.py.  Legs, interleaved round by round:
  `map`      = lumahip_distortion_map_frames_device(_f16);
  `replaced` = lumahip_encode_frames_device(_f16) into scratch planes, then the torch reduction per block that yields the same words
               (difference, pad to whole blocks, reshape into blocks, square, sum, amax, count per plane);
  `frame`    = lumahip_distortion_frames_device(_f16) on the same inputs: twelve words per frame, one memset and global atomics.
Per leg and round: hipEvent time of back-to-back launches, at least --min-s seconds of device time; the median round is reported.
The integers of `map` and `replaced` are compared once before anything is timed, and the map folded per frame against `frame`.
-> profiles/distortion_map.jsonl: every run APPENDS one JSON line with, per workload and block size, ms and Mpixel/s of each leg, map
over replaced (the bar: >= 1), map's time over frame's (recorded; block 64 against 16 shows the tail of the few map tiles), and the
spread of the rounds."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import lumahdrv_amd as L  # noqa: E402
from lumahdrv_amd import capi  # noqa: E402

CFG = {"pq11_luv8": ((L.PTF_PQ, 11, L.CS_LUV, 8, 1e4, 0.005), 1.0),
       "pq10_ycbcr10": ((L.PTF_PQ, 10, L.CS_YCBCR, 10, 1000.0, 0.01), 20.0)}
WORKLOADS = [("pq11_luv8", False), ("pq11_luv8", True), ("pq10_ycbcr10", True)]   # (configuration, frames of halves)
BLOCKS = (16, 64)


def torch_block_reduction(e, g, B, dims, block, out):
    """the map from two sets of 16-bit 4:2:0 planes (uint8 tensors, B frames each, no padding; dims[p] = (rows, columns) of plane p)
    into out (B, nby, nbx, 3, 4)"""
    nby, nbx = out.shape[1], out.shape[2]
    for p in range(3):
        rows, cols = dims[p]
        b = block if p == 0 else block // 2
        d = ((e[p].view(torch.int16).to(torch.int32) & 0xFFFF) - (g[p].view(torch.int16).to(torch.int32) & 0xFFFF)).abs().view(B, rows, cols)
        d = torch.nn.functional.pad(d, (0, nbx * b - cols, 0, nby * b - rows)).view(B, nby, b, nbx, b)
        out[:, :, :, p, 0] = (d.to(torch.int64) ** 2).sum((2, 4))
        out[:, :, :, p, 1] = d.sum((2, 4), dtype=torch.int64)
        out[:, :, :, p, 2] = d.amax((2, 4))
        out[:, :, :, p, 3] = (d != 0).sum((2, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--min-s", type=float, default=1.0, help="device time per leg and round")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distortion_map.jsonl"), help="'' = print only")
    ap.add_argument("--only", default="", help="one workload, e.g. pq11_luv8:f32 or pq10_ycbcr10:f16 (for rocprofv3 captures)")
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
    rows = []
    for name, halves in WORKLOADS:
        tag = "%s:%s" % (name, "f16" if halves else "f32")
        if a.only and a.only != tag:
            continue
        cfg, sc = CFG[name]
        c = L.Context(0)
        c.set_stream(s.cuda_stream)
        c.set_quantizer(*cfg, L.build_lut(cfg[0], cfg[1], cfg[4], cfg[5]))
        if halves:
            c.tune("half_table", 2)   # the typed calls take the table whenever it exists; said here so that the encode leg does too
        f32 = torch.empty(nb * B * n3, dtype=torch.float32, device=dev)
        c.synth_frames_device(f32.data_ptr(), n3, nb * B, w, h)
        frames = f32.to(torch.float16) if halves else f32
        if halves:
            del f32
        given = [torch.zeros(nb * B * psz[p], dtype=torch.uint8, device=dev) for p in range(3)]
        scratch = [torch.zeros(B * psz[p], dtype=torch.uint8, device=dev) for p in range(3)]
        out_f = torch.zeros(nb, B, 3, 4, dtype=torch.int64, device=dev)
        esz = frames.element_size()
        enc = c.encode_frames_device_f16 if halves else c.encode_frames_device
        dist = c.distortion_frames_device_f16 if halves else c.distortion_frames_device
        dmap = c.distortion_map_frames_device_f16 if halves else c.distortion_map_frames_device

        def fr(b):
            return frames.data_ptr() + b * B * n3 * esz

        def at(t, b):
            return [t[p].data_ptr() + b * B * psz[p] for p in range(3)]

        for b in range(nb):
            enc(fr(b), n3, B, w, h, sc * 1.02, profile, at(given, b), st, psz)

        for block in BLOCKS:
            nbx, nby = capi.distortion_map_dims(w, h, block)
            out_m = torch.full((nb, B, nby, nbx, 3, 4), -1, dtype=torch.int64, device=dev)   # (the launch writes every word)
            out_r = torch.zeros(nb, B, nby, nbx, 3, 4, dtype=torch.int64, device=dev)

            def launch(leg, b):
                if leg == "map":
                    dmap(fr(b), n3, B, w, h, sc, profile, at(given, b), st, psz, block, out_m[b].data_ptr())
                elif leg == "frame":
                    dist(fr(b), n3, B, w, h, sc, profile, at(given, b), st, psz, out_f[b].data_ptr())
                else:
                    enc(fr(b), n3, B, w, h, sc, profile, [t.data_ptr() for t in scratch], st, psz)
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
                rows.append(dict(workload=tag, block=block, frames_per_launch=B, w=w, h=h, profile=profile, sc=sc,
                                 samples_differing=round(differing, 3), ms={leg: round(med[leg], 4) for leg in legs},
                                 mpixel_s={leg: round(mpx[leg], 1) for leg in legs}, map_over_replaced=round(mpx["map"] / mpx["replaced"], 3),
                                 map_ms_over_frame_ms=round(med["map"] / med["frame"], 3),
                                 spread={leg: round(max(v) / min(v) - 1, 4) for leg, v in res.items()}, launches_per_round=iters))
            del out_m, out_r
        c.close()
        del frames, given, scratch, out_f
        torch.cuda.empty_cache()
    for r in rows:
        print("%-18s block %2d: map %8.4f ms | replaced %8.4f ms | per-frame distortion %8.4f ms | map x%.3f of replaced | map / frame %.3f | "
              "spread %s" % (r["workload"], r["block"], r["ms"]["map"], r["ms"]["replaced"], r["ms"]["frame"], r["map_over_replaced"],
                             r["map_ms_over_frame_ms"], r["spread"]))
    if a.out and rows:
        line = dict(rounds=a.rounds, min_s=a.min_s, kernel_source_sha=capi.kernel_source_sha(), device=torch.cuda.get_device_name(0),
                    library=os.path.basename(os.path.dirname(capi.library_path())), workloads=rows)
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
