#!/usr/bin/env python3
"""tools/bench/f16_frames.py [--rounds R] [--iters N] [--out FILE] -- float32 against binary16 frames on a resident 4K stream.

Workloads: PQ-11 Lu'v' profile 2 (BASELINE's) and the HDR10 Y'CbCr recipe (PQ-10, 10-bit colour, sc 20), encode and decode,
8 frames of 3840x2160 per launch, ordered launches on one stream over four distinct batches (3 GiB of float frames: every launch
is fed from HBM).  Both frame types hold the same values (halves, widened for the float calls), so the float YCbCr encode
may take the half-input table too.  Per launch: hipEvent time of N back-to-back launches / N; rounds alternate float and f16.
Reports Mpixel/s and the fraction of 8 TB/s at each call's real bytes per pixel (frames 12 or 6, planes 3 for profile 2).
-> profiles/f16_frames.jsonl (one JSON line per workload / direction / frame type, the median round)"""
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
WORKLOADS = {"pq11_luv_p2": ((L.PTF_PQ, 11, L.CS_LUV, 8, 1e4, 0.005), 1.0),
             "hdr10_ycbcr_p2": ((L.PTF_PQ, 10, L.CS_YCBCR, 10, 1000.0, 0.01), 20.0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f16_frames.jsonl"), help="'' = print only")
    ap.add_argument("--only", default="", help="run one workload (for rocprofv3 captures)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    w, h, B, nb, profile = 3840, 2160, a.frames, 4, 2
    n, n3 = w * h, 3 * w * h
    _, hs, st, bps = L.plane_geometry(w, h, profile)
    psz = [hs[p] * st[p] for p in range(3)]
    plane_bpp = sum(psz) / n
    rows = []
    for wl, (cfg, sc) in WORKLOADS.items():
        if a.only and wl != a.only:
            continue
        ctx = L.Context(0)
        s = torch.cuda.current_stream()
        ctx.set_stream(s.cuda_stream)
        ctx.set_quantizer(*cfg, L.build_lut(cfg[0], cfg[1], cfg[4], cfg[5]))
        x32 = torch.empty(nb * B * n3, dtype=torch.float32, device=dev)
        ctx.synth_frames_device(x32.data_ptr(), n3, nb * B, w, h)
        x16 = x32.to(torch.float16)
        x32.copy_(x16.float())                       # the same values in both frame types
        planes = [torch.zeros(nb * B * psz[p], dtype=torch.uint8, device=dev) for p in range(3)]
        out32 = torch.empty(B * n3, dtype=torch.float32, device=dev)   # (one decode batch: the writes stream to HBM anyway)
        out16 = torch.empty(B * n3, dtype=torch.float16, device=dev)

        def pl(b):
            return [planes[p].data_ptr() + b * B * psz[p] for p in range(3)]

        def launch(d, half, b):
            if d == "encode":
                if half:
                    ctx.encode_frames_device_f16(x16.data_ptr() + b * B * n3 * 2, n3, B, w, h, sc, profile, pl(b), st, psz)
                else:
                    ctx.encode_frames_device(x32.data_ptr() + b * B * n3 * 4, n3, B, w, h, sc, profile, pl(b), st, psz)
            else:
                if half:
                    ctx.decode_frames_device_f16(pl(b), st, psz, B, w, h, profile, sc, out16.data_ptr(), n3)
                else:
                    ctx.decode_frames_device(pl(b), st, psz, B, w, h, profile, sc, out32.data_ptr(), n3)

        for b in range(nb):   # planes for the decode runs, and a warm-up of every variant
            launch("encode", False, b)
        for d in ("encode", "decode"):
            for half in (False, True):
                for b in range(nb):
                    launch(d, half, b)
        torch.cuda.synchronize()
        res = {}
        for r in range(a.rounds):
            for d in ("encode", "decode"):
                for half in ((False, True) if r % 2 == 0 else (True, False)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(s)
                    for i in range(a.iters):
                        launch(d, half, i % nb)
                    e1.record(s)
                    e1.synchronize()
                    res.setdefault((d, half), []).append(e0.elapsed_time(e1) / a.iters)
        for (d, half), ms in sorted(res.items()):
            ms = sorted(ms)
            med = ms[len(ms) // 2]
            frame_bpp = 6 if half else 12
            bpp = frame_bpp + plane_bpp
            px_s = B * n / (med * 1e-3)
            rows.append(dict(workload=wl, direction=d, frames="f16" if half else "f32", ms_per_launch=round(med, 4),
                             ms_min=round(ms[0], 4), frames_per_launch=B, mpixel_s=round(px_s / 1e6, 1), bytes_per_pixel=bpp,
                             hbm_fraction_8tbs=round(px_s * bpp / HBM, 3), rounds=a.rounds, iters=a.iters))
        ctx.close()
        del x32, x16, planes, out32, out16
        torch.cuda.empty_cache()
    meta = dict(kernel_source_sha=capi.kernel_source_sha(), device=torch.cuda.get_device_name(0), w=w, h=h)
    lines = [json.dumps(dict(r, **meta)) for r in rows]
    for r in rows:
        print("%-15s %-6s %s  %8.4f ms  %9.1f Mpx/s  %4.1f B/px  %.3f of 8 TB/s" %
              (r["workload"], r["direction"], r["frames"], r["ms_per_launch"], r["mpixel_s"], r["bytes_per_pixel"], r["hbm_fraction_8tbs"]))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
