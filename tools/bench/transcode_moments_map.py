#!/usr/bin/env python3
"""tools/bench/transcode_moments_map.py [--rounds R] [--min-s S] [--out FILE] -- the transcode moments map launch against what it
replaces and against the transcode distortion map launch.

Workloads: PQ-11 Lu'v' planes -> LOG-12 Lu'v' and -> the HDR10 Y'CbCr recipe (PQ-10, 10-bit colour, sc 20); profile 2 on both
sides, 8 frames of 3840x2160 per launch, ordered launches on one stream, plain allocations, one process on one box, four distinct
batches; blocks of 8 and of 64 luma pixels.  The given planes are the source planes' own transcode under a target preScaling 2 %
off, as in tools/bench/transcode_distortion_map.py.  Legs, interleaved round by round:
  `moments`  = lumahip_transcode_moments_map_frames_device at blocks 8 and 64;
  `replaced` = lumahip_transcode_frames_device into scratch planes, then the torch reduction per block that yields the same 15
               words (tools/bench/moments_map.py torch_block_moments);
  `map`      = lumahip_transcode_distortion_map_frames_device on the same inputs at blocks 16 and 64 (its smallest block stands
               beside the moments' smallest): the launch the moments kernels were made from.  Its code does not change with theirs,
               so this leg is also the yardstick between two builds on one box.
Per leg and round: hipEvent time of back-to-back launches, at least --min-s seconds of device time; the median round is reported.
Once before anything is timed: `moments` equals `replaced` word for word, and sum e^2 - 2 sum e g + sum g^2 at block 64 equals
`map`'s sse.
-> profiles/transcode_moments_map.jsonl: every run APPENDS one JSON line with, per workload, ms and Mpixel/s of each leg and block,
moments over replaced (the bar: >= 1; the exit status is 1 below it), moments' time over map's at block 64 and at the smallest
blocks (8 over 16), moments' time at block 8 over block 64 (recorded, not gated), and the spread of the rounds."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import lumahdrv_amd as L  # noqa: E402
from lumahdrv_amd import capi  # noqa: E402
from tools.bench.moments_map import torch_block_moments  # noqa: E402
from tools.bench.transcode_distortion import SRC, TARGETS  # noqa: E402

LEGS = [("moments", 8), ("moments", 64), ("replaced", 8), ("replaced", 64), ("map", 16), ("map", 64)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--min-s", type=float, default=1.0, help="device time per leg and round")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transcode_moments_map.jsonl"), help="'' = print only")
    ap.add_argument("--only", default="", help="one target, e.g. log12_luv8 (for rocprofv3 captures)")
    ap.add_argument("--leg", default="", help="moments:8, moments:64, replaced:8, replaced:64, map:16 or map:64: that leg only, one round, nothing written")
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
        for b in range(nb):
            c.transcode_frames_device(at(src, b), st, psz, profile, src_sc, B, w, h, at(given, b), st, psz, profile, dst_sc * 1.02)

        out = {}
        for leg, block in LEGS:   # (the launches write every word of theirs)
            nbx, nby = capi.moments_map_dims(w, h, block)
            out[leg, block] = torch.full((nb, B, nby, nbx, 3, 4 if leg == "map" else 5), -1, dtype=torch.int64, device=dev)

        def launch(leg, block, b):
            if leg == "moments":
                c.transcode_moments_map_frames_device(at(src, b), st, psz, profile, src_sc, B, w, h, at(given, b), st, psz, profile, dst_sc,
                                                      block, out[leg, block][b].data_ptr())
            elif leg == "map":
                c.transcode_distortion_map_frames_device(at(src, b), st, psz, profile, src_sc, B, w, h, at(given, b), st, psz, profile,
                                                         dst_sc, block, out[leg, block][b].data_ptr())
            else:
                c.transcode_frames_device(at(src, b), st, psz, profile, src_sc, B, w, h, [t.data_ptr() for t in scratch], st, psz, profile,
                                          dst_sc)
                torch_block_moments(scratch, [given[p][b * B * psz[p]:(b + 1) * B * psz[p]] for p in range(3)], B, dims, block,
                                    out[leg, block][b])

        for b in range(nb):   # the methods compute the same integers
            for leg, block in LEGS:
                launch(leg, block, b)
        torch.cuda.synchronize()
        for block in (8, 64):
            if not torch.equal(out["moments", block], out["replaced", block]):
                raise SystemExit("%s, block %d: the moments launch and the replaced method disagree" % (tag, block))
        m64 = out["moments", 64]
        if not torch.equal(m64[..., 2] - 2 * m64[..., 4] + m64[..., 3], out["map", 64][..., 0]):
            raise SystemExit("%s: sum e^2 - 2 sum e g + sum g^2 is not the transcode distortion map's sse at block 64" % tag)
        differing = float(out["map", 64][..., 3].sum()) / (nb * B * 1.5 * n)

        def timed(leg, block, iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for i in range(iters):
                launch(leg, block, i % nb)
            e1.record(s)
            e1.synchronize()
            return e0.elapsed_time(e1) / iters

        legs = [lb for lb in LEGS if not a.leg or a.leg == "%s:%d" % lb]
        if not legs:
            raise SystemExit("--leg: one of " + ", ".join("%s:%d" % lb for lb in LEGS))
        iters = {}
        for lb in legs:   # warm-up, and how many launches make --min-s of device time
            timed(*lb, 4)
            iters[lb] = max(4, int(a.min_s * 1e3 / timed(*lb, 8)) + 1)
        res = {lb: [] for lb in legs}
        for r in range(1 if a.leg else a.rounds):
            for lb in (legs if r % 2 == 0 else legs[::-1]):
                res[lb].append(timed(*lb, iters[lb]))
        if a.leg:
            print("%s  %s: %.4f ms per launch" % (tag, a.leg, res[legs[0]][0]))
        else:
            med = {lb: sorted(v)[len(v) // 2] for lb, v in res.items()}
            key = "%s_%d".__mod__
            rows.append(dict(workload=tag, frames_per_launch=B, w=w, h=h, profile=profile, src_sc=src_sc, dst_sc=dst_sc,
                             samples_differing=round(differing, 3),
                             ms={key(lb): round(med[lb], 4) for lb in legs},
                             mpixel_s={key(lb): round(B * n / (med[lb] * 1e-3) / 1e6, 1) for lb in legs},
                             moments_over_replaced={str(b): round(med["replaced", b] / med["moments", b], 3) for b in (8, 64)},
                             moments_ms_over_map_ms_64=round(med["moments", 64] / med["map", 64], 3),
                             moments_ms_8_over_map_ms_16=round(med["moments", 8] / med["map", 16], 3),
                             moments_ms_8_over_64=round(med["moments", 8] / med["moments", 64], 3),
                             spread={key(lb): round(max(v) / min(v) - 1, 4) for lb, v in res.items()},
                             launches_per_round={key(lb): iters[lb] for lb in legs}))
        c.close()
        del given, scratch, out
        torch.cuda.empty_cache()
    for r in rows:
        print("%-26s moments %8.4f / %8.4f ms (block 8 / 64) | replaced %9.4f / %9.4f ms | distortion map %8.4f / %8.4f ms (16 / 64) | "
              "moments x%.3f / x%.3f of replaced | moments / map at 64 %.3f, at 8 / 16 %.3f | moments 8 / 64 %.3f" %
              (r["workload"], r["ms"]["moments_8"], r["ms"]["moments_64"], r["ms"]["replaced_8"], r["ms"]["replaced_64"], r["ms"]["map_16"],
               r["ms"]["map_64"], r["moments_over_replaced"]["8"], r["moments_over_replaced"]["64"], r["moments_ms_over_map_ms_64"],
               r["moments_ms_8_over_map_ms_16"], r["moments_ms_8_over_64"]))
    if a.out and rows:
        line = dict(rounds=a.rounds, min_s=a.min_s, kernel_source_sha=capi.kernel_source_sha(), device=torch.cuda.get_device_name(0),
                    library=os.path.basename(os.path.dirname(capi.library_path())), workloads=rows)
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")
    if any(min(r["moments_over_replaced"].values()) < 1.0 for r in rows):
        raise SystemExit(1)


if __name__ == "__main__":
    main()
