#!/usr/bin/env python3
"""tools/bench/distortion.py [--rounds R] [--min-s S] [--out FILE] -- the fused distortion launch against what it replaces.

Workloads: PQ-11 Lu'v' from float frames, PQ-11 Lu'v' from binary16 frames, the HDR10 Y'CbCr recipe (PQ-10, 10-bit colour, sc 20)
from binary16 frames; profile 2, 8 frames of 3840x2160 per launch, ordered launches on one stream, plain allocations, one process
on one box, four distinct batches.  The given planes are the frames' own planes under a preScaling 2 % off (small differences
nearly everywhere, as a lossy decode leaves them).  Legs, interleaved round by round:
  `fused`    = lumahip_distortion_frames_device(_f16);
  `replaced` = lumahip_encode_frames_device(_f16) into scratch planes, then the torch reduction that yields the same twelve
               integers per frame (difference, square, sum, max, count per plane);
  `encode`   = that encode launch alone (the kernel the fused one shares its first two stages with).
Per leg and round: hipEvent time of back-to-back launches, at least --min-s seconds of device time; the median round is reported.
The two legs' integers are compared once before anything is timed.
-> profiles/distortion.jsonl: every run APPENDS one JSON line with, per workload, ms and Mpixel/s of each leg, fused over replaced,
the fused and the encode kernel's fraction of 8 TB/s at their 15 (floats) / 9 (halves) B/pixel, and the spread of the rounds."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import lumahdrv_amd as L  # noqa: E402
from lumahdrv_amd import capi  # noqa: E402

HBM = 8e12
CFG = {"pq11_luv8": ((L.PTF_PQ, 11, L.CS_LUV, 8, 1e4, 0.005), 1.0),
       "pq10_ycbcr10": ((L.PTF_PQ, 10, L.CS_YCBCR, 10, 1000.0, 0.01), 20.0)}
WORKLOADS = [("pq11_luv8", False), ("pq11_luv8", True), ("pq10_ycbcr10", True)]   # (configuration, frames of halves)


def torch_reduction(e, g, B, out):
    """the twelve integers per frame from two sets of 16-bit planes (uint8 tensors, B frames each, no padding) into out (B, 3, 4)"""
    for p in range(3):
        d = ((e[p].view(torch.int16).to(torch.int32) & 0xFFFF) - (g[p].view(torch.int16).to(torch.int32) & 0xFFFF)).abs().view(B, -1)
        out[:, p, 0] = (d.to(torch.int64) ** 2).sum(1)
        out[:, p, 1] = d.sum(1, dtype=torch.int64)
        out[:, p, 2] = d.amax(1)
        out[:, p, 3] = (d != 0).sum(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--min-s", type=float, default=1.0, help="device time per leg and round")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distortion.jsonl"), help="'' = print only")
    ap.add_argument("--only", default="", help="one workload, e.g. pq11_luv8:f32 or pq10_ycbcr10:f16 (for rocprofv3 captures)")
    ap.add_argument("--leg", default="", help="fused, replaced or encode: that leg only, one round, nothing written")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    w, h, B, nb, profile = 3840, 2160, a.frames, 4, 2
    n, n3 = w * h, 3 * w * h
    _, hs, st, _ = L.plane_geometry(w, h, profile)
    psz = [hs[p] * st[p] for p in range(3)]
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
        out_r = torch.zeros(nb, B, 3, 4, dtype=torch.int64, device=dev)
        esz = frames.element_size()
        enc = c.encode_frames_device_f16 if halves else c.encode_frames_device
        dist = c.distortion_frames_device_f16 if halves else c.distortion_frames_device

        def fr(b):
            return frames.data_ptr() + b * B * n3 * esz

        def at(t, b):
            return [t[p].data_ptr() + b * B * psz[p] for p in range(3)]

        for b in range(nb):
            enc(fr(b), n3, B, w, h, sc * 1.02, profile, at(given, b), st, psz)

        def launch(leg, b):
            if leg == "fused":
                dist(fr(b), n3, B, w, h, sc, profile, at(given, b), st, psz, out_f[b].data_ptr())
                return
            enc(fr(b), n3, B, w, h, sc, profile, [t.data_ptr() for t in scratch], st, psz)
            if leg == "replaced":
                torch_reduction(scratch, [given[p][b * B * psz[p]:(b + 1) * B * psz[p]] for p in range(3)], B, out_r[b])

        for b in range(nb):   # the two legs compute the same integers
            launch("fused", b)
            launch("replaced", b)
        torch.cuda.synchronize()
        if not torch.equal(out_f, out_r):
            raise SystemExit("%s: the fused launch and the replaced method disagree" % tag)
        differing = float(out_f[..., 3].sum()) / (nb * B * 1.5 * n)

        def timed(leg, iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for i in range(iters):
                launch(leg, i % nb)
            e1.record(s)
            e1.synchronize()
            return e0.elapsed_time(e1) / iters

        legs = [a.leg] if a.leg else ["fused", "replaced", "encode"]
        iters = {}
        for leg in legs:   # warm-up, and how many launches make --min-s of device time
            timed(leg, 4)
            iters[leg] = max(4, int(a.min_s * 1e3 / timed(leg, 8)) + 1)
        res = {leg: [] for leg in legs}
        for r in range(1 if a.leg else a.rounds):
            for leg in (legs if r % 2 == 0 else legs[::-1]):
                res[leg].append(timed(leg, iters[leg]))
        if a.leg:
            print("%s  %s: %.4f ms per launch" % (tag, a.leg, res[a.leg][0]))
        else:
            med = {leg: sorted(v)[len(v) // 2] for leg, v in res.items()}
            mpx = {leg: B * n / (med[leg] * 1e-3) / 1e6 for leg in legs}
            bpp = 9 if halves else 15
            rows.append(dict(workload=tag, frames_per_launch=B, w=w, h=h, profile=profile, sc=sc, samples_differing=round(differing, 3),
                             ms={leg: round(med[leg], 4) for leg in legs}, mpixel_s={leg: round(mpx[leg], 1) for leg in legs},
                             fused_over_replaced=round(mpx["fused"] / mpx["replaced"], 3), bytes_per_pixel=bpp,
                             fused_hbm_fraction_8tbs=round(mpx["fused"] * 1e6 * bpp / HBM, 3),
                             encode_hbm_fraction_8tbs=round(mpx["encode"] * 1e6 * bpp / HBM, 3),
                             spread={leg: round(max(v) / min(v) - 1, 4) for leg, v in res.items()}, launches_per_round=iters))
        c.close()
        del frames, given, scratch, out_f, out_r
        torch.cuda.empty_cache()
    for r in rows:
        print("%-18s fused %8.4f ms | replaced %8.4f ms | encode alone %8.4f ms | fused x%.3f of replaced | of 8 TB/s at %d B/px: fused %.3f, "
              "encode %.3f | spread %s" % (r["workload"], r["ms"]["fused"], r["ms"]["replaced"], r["ms"]["encode"], r["fused_over_replaced"],
                                           r["bytes_per_pixel"], r["fused_hbm_fraction_8tbs"], r["encode_hbm_fraction_8tbs"], r["spread"]))
    if a.out and rows:
        line = dict(rounds=a.rounds, min_s=a.min_s, kernel_source_sha=capi.kernel_source_sha(), device=torch.cuda.get_device_name(0),
                    workloads=rows)
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
