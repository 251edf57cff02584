#!/usr/bin/env python3
"""tools/bench/light_level.py [--rounds R] [--min-s S] [--out FILE] [--sweep] [--leg NAME] -- the content light level launches
(include/lumahip_compare.h) against the methods they replace and against the launches that move the same bytes.

8 frames of 3840x2160 per launch, ordered launches on one stream, plain allocations, one process on one box, four distinct batches.
Legs, interleaved round by round:
  frame-fed
    `light_f32` / `light_f16`   lumahip_light_level_frames_device / _f16 on float / binary16 frames (12 / 6 B per pixel), scale 1;
    `torch_f32` / `torch_f16`   the replaced method: torch on the same frames -- scale, the maximum over the channels, the Y row, * 256,
                                the three cases of q, integer sum / max / counts per frame (halves are widened first, which is part
                                of what it costs);
    `encode_f32`                the reference launch: lumahip_encode_frames_device (PQ-11 Lu'v', profile 2) on the same float frames --
                                the same 12 B per pixel read, 3 written and the whole encode arithmetic; its code is the parent's;
  plane-fed, for PQ-11 Lu'v' planes (`luv`, sc 1) and HDR10 planes (`hdr10`: PQ-10 YCbCr, sc 20), profile 2, 3 B per pixel, scale = sc
    `planes_X`                  lumahip_planes_light_level_frames_device;
    `decode_torch_X`            the replaced method: lumahip_decode_frames_device into scratch float frames + the same torch reduction;
    `decode_X`                  the reference launch: that decode launch alone.
Per leg and round: hipEvent time of back-to-back launches, at least --min-s seconds of device time; the median round is reported.
Once before anything is timed: every method gives the same eight integers per frame.
--sweep: additionally lumahip_tune("blocks_per_cu") over {3, 5, 8} on the four fused legs, the values interleaved round by round, the
median of the rounds per value (a quarter of --min-s each); goes into the line.
-> profiles/light_level.jsonl: every run APPENDS one JSON line with ms per launch of each leg, the ratios, the fractions of 8 TB/s at
12 / 6 / 3 B per pixel and the spread of the rounds.
Gates, on the medians with the larger of the two legs' round spread as margin; the exit status is 3 below any:
  1. every fused leg is no slower than the method it replaces;
  2. `light_f32` is no slower than `encode_f32`.
--leg NAME runs that leg alone, one round, nothing written (for a counters capture)."""
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
LUV = (L.PTF_PQ, 11, L.CS_LUV, 8, 1e4, 0.005)
HDR10 = (L.PTF_PQ, 10, L.CS_YCBCR, 10, 1000.0, 0.01)
PLANE_STREAMS = {"luv": (LUV, 1.0), "hdr10": (HDR10, 20.0)}
PROFILE = 2
SWEEP = (3, 5, 8)
OVER = 0xFFFFFFFF


def torch_light(x, scale, out):
    """the eight words per frame of x, (B, 3, h, w) float32 or float16, into out, (B, 8) int64: plain torch, one rounded fp32
    operation per step as the statistic states them"""
    x = x.float()
    if scale != 1.0:
        x = x * scale
    r, g, b = x[:, 0], x[:, 1], x[:, 2]
    m = torch.fmax(torch.fmax(r, g), b)
    y = (0.212656 * r + 0.715158 * g) + 0.072186 * b
    for k, v in enumerate((m, y)):
        t = v * 256.0
        over = t >= 4294967296.0
        mid = (t > 0) & ~over
        q = torch.where(mid, t, 0.0).floor().to(torch.int64)
        q = torch.where(over, OVER, q)
        out[:, 4 * k + 0] = q.sum(dim=(1, 2))
        out[:, 4 * k + 1] = q.amax(dim=(1, 2))
        out[:, 4 * k + 2] = over.sum(dim=(1, 2))
        out[:, 4 * k + 3] = torch.isnan(v).sum(dim=(1, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--min-s", type=float, default=1.0, help="device time per leg and round")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "light_level.jsonl"), help="'' = print only")
    ap.add_argument("--leg", default="", help="that leg only, one round, nothing written")
    ap.add_argument("--sweep", action="store_true", help="+ blocks_per_cu over {3, 5, 8} on the fused legs")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    w, h, B, nb = 3840, 2160, a.frames, 4
    n, n3 = w * h, 3 * w * h
    s = torch.cuda.current_stream()

    def context(cfg):
        c = L.Context(0)
        c.set_stream(s.cuda_stream)
        if cfg is not None:
            c.set_quantizer(*cfg, L.build_lut(cfg[0], cfg[1], cfg[4], cfg[5]))
        return c

    bare = context(None)                     # the frame-fed calls run on a context without a quantizer
    ctxs = {name: context(cfg) for name, (cfg, _) in PLANE_STREAMS.items()}
    f32 = torch.empty(nb * B * n3, dtype=torch.float32, device=dev)
    ctxs["luv"].synth_frames_device(f32.data_ptr(), n3, nb * B, w, h)
    f16 = f32.half()
    _, hs, st, _ = L.plane_geometry(w, h, PROFILE)
    psz = [hs[p] * st[p] for p in range(3)]
    planes = {name: [torch.zeros(nb * B * psz[p], dtype=torch.uint8, device=dev) for p in range(3)] for name in PLANE_STREAMS}
    enc_dst = [torch.zeros(B * psz[p], dtype=torch.uint8, device=dev) for p in range(3)]
    scratch = torch.empty(B * n3, dtype=torch.float32, device=dev)

    def at(t, b):
        return [t[p].data_ptr() + b * B * psz[p] for p in range(3)]

    def frames32(b):
        return f32[b * B * n3:(b + 1) * B * n3].view(B, 3, h, w)

    def frames16(b):
        return f16[b * B * n3:(b + 1) * B * n3].view(B, 3, h, w)

    for name, (_, sc) in PLANE_STREAMS.items():
        for b in range(nb):
            ctxs[name].encode_frames_device(f32.data_ptr() + b * B * n3 * 4, n3, B, w, h, sc, PROFILE, at(planes[name], b), st, psz)

    legs = ["light_f32", "torch_f32", "encode_f32", "light_f16", "torch_f16"]
    for name in PLANE_STREAMS:
        legs += ["planes_" + name, "decode_torch_" + name, "decode_" + name]
    out = {lg: torch.full((nb, B, 8), -1, dtype=torch.int64, device=dev) for lg in legs if lg.startswith(("light_", "torch_", "planes_", "decode_torch_"))}

    def launch(lg, b):
        if lg == "light_f32":
            bare.light_level_frames_device(f32.data_ptr() + b * B * n3 * 4, n3, B, w, h, 1.0, out[lg][b].data_ptr())
        elif lg == "light_f16":
            bare.light_level_frames_device_f16(f16.data_ptr() + b * B * n3 * 2, n3, B, w, h, 1.0, out[lg][b].data_ptr())
        elif lg == "torch_f32":
            torch_light(frames32(b), 1.0, out[lg][b])
        elif lg == "torch_f16":
            torch_light(frames16(b), 1.0, out[lg][b])
        elif lg == "encode_f32":
            ctxs["luv"].encode_frames_device(f32.data_ptr() + b * B * n3 * 4, n3, B, w, h, 1.0, PROFILE, [t.data_ptr() for t in enc_dst], st, psz)
        else:
            kind, name = lg.rsplit("_", 1)
            c, sc = ctxs[name], PLANE_STREAMS[name][1]
            if kind == "planes":
                c.planes_light_level_frames_device(at(planes[name], b), st, psz, B, w, h, PROFILE, sc, sc, out[lg][b].data_ptr())
            else:
                c.decode_frames_device(at(planes[name], b), st, psz, B, w, h, PROFILE, sc, scratch.data_ptr(), n3)
                if kind == "decode_torch":
                    torch_light(scratch.view(B, 3, h, w), sc, out[lg][b])

    for b in range(nb):   # the methods compute the same integers
        for lg in legs:
            launch(lg, b)
    torch.cuda.synchronize()
    pairs = [("light_f32", "torch_f32"), ("light_f16", "torch_f16")] + [("planes_" + nm, "decode_torch_" + nm) for nm in PLANE_STREAMS]
    for fused, replaced in pairs:
        if not torch.equal(out[fused], out[replaced]):
            raise SystemExit("`%s` and `%s` disagree" % (fused, replaced))
        if not (out[fused][..., [0, 1, 4, 5]] > 0).all():
            raise SystemExit("`%s`: a frame without light" % fused)

    def timed(lg, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for i in range(iters):
            launch(lg, i % nb)
        e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1) / iters

    if a.leg:
        if a.leg not in legs:
            raise SystemExit("--leg: one of %s" % legs)
        legs = [a.leg]
    iters = {}
    for lg in legs:   # warm-up, and how many launches make --min-s of device time
        timed(lg, 4)
        iters[lg] = max(4, int(a.min_s * 1e3 / timed(lg, 8)) + 1)
    res = {lg: [] for lg in legs}
    for r in range(1 if a.leg else a.rounds):
        for lg in (legs if r % 2 == 0 else legs[::-1]):
            res[lg].append(timed(lg, iters[lg]))
    if a.leg:
        print("%s: %.4f ms per launch" % (a.leg, res[a.leg][0]))
        return
    med = {lg: sorted(v)[len(v) // 2] for lg, v in res.items()}
    spread = {lg: max(v) / min(v) - 1 for lg, v in res.items()}
    read_bytes = {"light_f32": 12, "light_f16": 6, "planes_luv": 3, "planes_hdr10": 3}
    fused = list(read_bytes)
    gates = {}
    for fz, other in pairs + [("light_f32", "encode_f32")]:
        gates["%s_no_slower_than_%s" % (fz, other)] = bool(med[fz] <= med[other] * (1 + max(spread[fz], spread[other])))
    line = dict(rounds=a.rounds, min_s=a.min_s, kernel_source_sha=capi.kernel_source_sha(), device=torch.cuda.get_device_name(0),
                library=os.path.basename(os.path.dirname(capi.library_path())), frames_per_launch=B, w=w, h=h, profile=PROFILE,
                ms={lg: round(med[lg], 4) for lg in legs}, spread={lg: round(spread[lg], 4) for lg in legs},
                launches_per_round=iters,
                replaced_over_fused={fz: round(med[other] / med[fz], 3) for fz, other in pairs},
                fused_over_reference={"light_f32": round(med["light_f32"] / med["encode_f32"], 3),
                                      **{"planes_" + nm: round(med["planes_" + nm] / med["decode_" + nm], 3) for nm in PLANE_STREAMS}},
                fraction_of_8TBs={lg: round(B * n * bpp / (med[lg] * 1e-3) / HBM, 3) for lg, bpp in read_bytes.items()},
                gates=gates)
    if a.sweep:
        tuned = {"light_f32": bare, "light_f16": bare, "planes_luv": ctxs["luv"], "planes_hdr10": ctxs["hdr10"]}
        sw = {(v, lg): [] for v in SWEEP for lg in fused}
        for r in range(a.rounds):
            for v in (SWEEP if r % 2 == 0 else SWEEP[::-1]):
                for c in set(tuned.values()):
                    c.tune("blocks_per_cu", v)
                for lg in fused:
                    sw[v, lg].append(timed(lg, max(4, iters[lg] // 4)))
        for c in set(tuned.values()):
            c.tune("blocks_per_cu", 0)
        line["blocks_per_cu_sweep_ms"] = {lg: {str(v): round(sorted(sw[v, lg])[len(sw[v, lg]) // 2], 4) for v in SWEEP} for lg in fused}
        line["blocks_per_cu_sweep_spread"] = {lg: {str(v): round(max(sw[v, lg]) / min(sw[v, lg]) - 1, 4) for v in SWEEP} for lg in fused}
    for lg in legs:
        print("%-20s %9.4f ms  (spread %.3f)%s" % (lg, med[lg], spread[lg],
                                                   "  %.3f of 8 TB/s" % line["fraction_of_8TBs"][lg] if lg in read_bytes else ""))
    if a.sweep:
        print("blocks_per_cu sweep (ms): %s" % json.dumps(line["blocks_per_cu_sweep_ms"]))
    print("gates: %s" % json.dumps(gates))
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")
    if not all(gates.values()):
        print("gates failed: %s" % [k for k, ok in gates.items() if not ok])
        raise SystemExit(3)


if __name__ == "__main__":
    main()
