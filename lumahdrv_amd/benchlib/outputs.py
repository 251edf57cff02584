"""`bench.py --dump-outputs DIR`: what the timed path computed in its last step, as float32 .npy files.

The timed step is one encode launch over a batch of B frames; what its caller receives are the batch's Y, U and V planes
(16-bit codes for profile 2, 8-bit for profiles 0 / 1).  A 4K batch holds 166 M luma codes, so each plane is written as a
fixed, seeded sample of its valid samples (stride padding excluded): the same arguments give the same positions in every
run and every build, so two dumps compare element for element.  A plane with no more samples than its cap is written whole.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from .plan import SEED

PLANE_NAMES = ("y", "u", "v")
SAMPLE_CAP = (4 << 20, 1 << 20, 1 << 20)       # samples per plane: 24 MB of float32 in all, under the 64 MB limit


def sample_positions(n, cap, p):
    """indices into the n valid samples of plane p, in ascending order: all of them when n <= cap, else a seeded sample"""
    if n <= cap:
        return np.arange(n, dtype=np.int64)
    rng = np.random.default_rng([SEED, p])
    return np.sort(rng.integers(0, n, cap, dtype=np.int64))


def plane_samples(plane_ptrs, B, w, h, profile, dev):
    """{name: float32 array} of the Y / U / V planes of one batch (B frames, vpx_img_alloc(fmt(profile), w, h, 32) layout,
    frame stride = one frame's plane bytes) at the positions of sample_positions"""
    from lumahdrv_amd import capi
    from lumahdrv_amd.placement import as_tensor
    ws, hs, st, bps = capi.plane_geometry(w, h, profile)
    out = {}
    for p in range(3):
        psz = hs[p] * st[p]
        raw = as_tensor(plane_ptrs[p], B * psz, dev)
        codes = raw.view(torch.int16) if bps == 2 else raw
        i = sample_positions(B * hs[p] * ws[p], SAMPLE_CAP[p], p)
        f, rem = np.divmod(i, hs[p] * ws[p])
        r, c = np.divmod(rem, ws[p])
        elem = torch.from_numpy(f * (psz // bps) + r * (st[p] // bps) + c).to(dev)
        v = codes[elem].to(torch.int32)
        if bps == 2:
            v = v & 0xFFFF
        out["%s_plane_sample" % PLANE_NAMES[p]] = v.to(torch.float32).cpu().numpy()
    return out


def write_outputs(d, arrays):
    os.makedirs(d, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(d, name + ".npy"), np.ascontiguousarray(a, dtype=np.float32))
