"""What the test modules share.  A test module imports its helpers from here and never from another test module; nothing in this package
is collected as a test.

host.py    numpy alone (no torch, no library): the plane geometry, the numpy models the measuring calls are held to
           (expected_distortion, expected_distortion_map, fold_map, float_to_half_np, the half-table policy), the readers of the
           fixtures in tests/golden, perturb and its kin, the constants (SENTINEL, GAP, GUARD, OUT_FILL, BLOCKS, the shared
           configurations and sizes), and the pure builders of the host byte buffers behind Frames and Planes.
device.py  the `L` fixture (test modules import it by name), dev, ctx, table_for, pair; Frames and Planes in device buffers, from_frames,
           random_planes, the out-word and map buffers; one wrapper per device call (encode, dist, dist_map, fused, two_calls,
           transcoded, measure, tmap).  torch is imported inside the functions.
display.py numpy alone: the display transform in float64 kept before its floor (display_t), what an RGBA image must satisfy against
           it (check_rgba, with the derivation of its EPS), the conditions on a reference image and frames that meet them.
exr.py     an OpenEXR scan-line writer and reader in numpy + zlib.
tools.py   ROOT, and what runs as a process of its own: bench.py, the facade's round-trip program.

pytest rewrites `assert` in test modules only, so every assert in this package carries its own message.
"""
