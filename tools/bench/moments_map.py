#!/usr/bin/env python3
"""tools/bench/moments_map.py [--rounds R] [--min-s S] [--out FILE] -- the moments map launch against what it replaces and against
the distortion map launch.

Workloads: PQ-11 Lu'v' from float frames, PQ-11 Lu'v' from binary16 frames, the HDR10 Y'CbCr recipe (PQ-10, 10-bit colour, sc 20)
from binary16 frames; profile 2, 8 frames of 3840x2160 per launch, ordered launches on one stream, plain allocations, one process
on one box, four distinct batches; blocks of 8 and of 64 luma pixels.  The given planes are the frames' own planes under a
preScaling 2 % off, as in tools/bench/distortion_map.py.  Legs, interleaved round by round:
  `moments`  = lumahip_moments_map_frames_device(_f16) at blocks 8 and 64;
  `replaced` = lumahip_encode_frames_device(_f16) into scratch planes, then the torch reduction per block that yields the same 15
               words (widen, square, multiply, pad to whole blocks, reshape into blocks, sum per plane);
  `map`      = lumahip_distortion_map_frames_device(_f16) on the same inputs at blocks 16 and 64 (its smallest block stands beside
               the moments' smallest): the launch the moments kernels were made from.
Per leg and round: hipEvent time of back-to-back launches, at least --min-s seconds of device time; the median round is reported.
Once before anything is timed: `moments` equals `replaced` word for word, and sum e^2 - 2 sum e g + sum g^2 at block 64 equals
`map`'s sse.
-> profiles/moments_map.jsonl: every run APPENDS one JSON line with, per workload, ms and Mpixel/s of each leg and block, moments
over replaced (the bar: >= 1; the exit status is 1 below it), moments' time over map's at block 64 and moments' time at block 8 over
block 64 (both recorded, not gated), and the spread of the rounds."""
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
LEGS = [("moments", 8), ("moments", 64), ("replaced", 8), ("replaced", 64), ("map", 16), ("map", 64)]


def torch_block_moments(e, g, B, dims, block, out):
    """the moments map from two sets of 16-bit 4:2:0 planes (uint8 tensors, B frames each, no padding; dims[p] = (rows, columns) of
    plane p) into out (B, nby, nbx, 3, 5)"""
    nby, nbx = out.shape[1], out.shape[2]
    for p in range(3):
        rows, cols = dims[p]
        b = block if p == 0 else block // 2
        ev = (e[p].view(torch.int16).to(torch.int64) & 0xFFFF).view(B, rows, cols)
        gv = (g[p].view(torch.int16).to(torch.int64) & 0xFFFF).view(B, rows, cols)
        for k, v in enumerate((ev, gv, ev * ev, gv * gv, ev * gv)):
            out[:, :, :, p, k] = torch.nn.functional.pad(v, (0, nbx * b - cols, 0, nby * b - rows)).view(B, nby, b, nbx, b).sum((2, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--min-s", type=float, default=1.0, help="device time per leg and round")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moments_map.jsonl"), help="'' = print only")
    ap.add_argument("--only", default="", help="one workload, e.g. pq11_luv8:f32 or pq10_ycbcr10:f16 (for rocprofv3 captures)")
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
        esz = frames.element_size()
        enc = c.encode_frames_device_f16 if halves else c.encode_frames_device
        mom = c.moments_map_frames_device_f16 if halves else c.moments_map_frames_device
        dmap = c.distortion_map_frames_device_f16 if halves else c.distortion_map_frames_device

        def fr(b):
            return frames.data_ptr() + b * B * n3 * esz

        def at(t, b):
            return [t[p].data_ptr() + b * B * psz[p] for p in range(3)]

        for b in range(nb):
            enc(fr(b), n3, B, w, h, sc * 1.02, profile, at(given, b), st, psz)

        out = {}
        for leg, block in LEGS:   # (the launches write every word of theirs)
            nbx, nby = capi.moments_map_dims(w, h, block)
            out[leg, block] = torch.full((nb, B, nby, nbx, 3, 4 if leg == "map" else 5), -1, dtype=torch.int64, device=dev)

        def launch(leg, block, b):
            if leg == "moments":
                mom(fr(b), n3, B, w, h, sc, profile, at(given, b), st, psz, block, out[leg, block][b].data_ptr())
            elif leg == "map":
                dmap(fr(b), n3, B, w, h, sc, profile, at(given, b), st, psz, block, out[leg, block][b].data_ptr())
            else:
                enc(fr(b), n3, B, w, h, sc, profile, [t.data_ptr() for t in scratch], st, psz)
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
            raise SystemExit("%s: sum e^2 - 2 sum e g + sum g^2 is not the distortion map's sse at block 64" % tag)

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
            rows.append(dict(workload=tag, frames_per_launch=B, w=w, h=h, profile=profile, sc=sc,
                             ms={key(lb): round(med[lb], 4) for lb in legs},
                             mpixel_s={key(lb): round(B * n / (med[lb] * 1e-3) / 1e6, 1) for lb in legs},
                             moments_over_replaced={str(b): round(med["replaced", b] / med["moments", b], 3) for b in (8, 64)},
                             moments_ms_over_map_ms_64=round(med["moments", 64] / med["map", 64], 3),
                             moments_ms_8_over_64=round(med["moments", 8] / med["moments", 64], 3),
                             map_ms_16_over_64=round(med["map", 16] / med["map", 64], 3),
                             spread={key(lb): round(max(v) / min(v) - 1, 4) for lb, v in res.items()},
                             launches_per_round={key(lb): iters[lb] for lb in legs}))
        c.close()
        del frames, given, scratch, out
        torch.cuda.empty_cache()
    for r in rows:
        print("%-18s moments %8.4f / %8.4f ms (block 8 / 64) | replaced %9.4f / %9.4f ms | distortion map %8.4f / %8.4f ms (16 / 64) | "
              "moments x%.3f / x%.3f of replaced | moments / map at 64 %.3f | moments 8 / 64 %.3f" %
              (r["workload"], r["ms"]["moments_8"], r["ms"]["moments_64"], r["ms"]["replaced_8"], r["ms"]["replaced_64"], r["ms"]["map_16"],
               r["ms"]["map_64"], r["moments_over_replaced"]["8"], r["moments_over_replaced"]["64"], r["moments_ms_over_map_ms_64"],
               r["moments_ms_8_over_64"]))
    if a.out and rows:
        line = dict(rounds=a.rounds, min_s=a.min_s, kernel_source_sha=capi.kernel_source_sha(), device=torch.cuda.get_device_name(0),
                    library=os.path.basename(os.path.dirname(capi.library_path())), workloads=rows)
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")
    if any(min(r["moments_over_replaced"].values()) < 1.0 for r in rows):
        raise SystemExit(1)


if __name__ == "__main__":
    main()
