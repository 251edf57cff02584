"""What the tests start as processes of their own: bench.py, and the C++ facade's round-trip program."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def bench(*flags, env=None):
    e = dict(os.environ)
    e.update(env or {})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(flags), capture_output=True, text=True, env=e, timeout=900)
    return p


def build_facade_test(tmp):
    exe = os.path.join(tmp, "facade_roundtrip")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "facade_roundtrip.cpp"), "-o", exe,
                    "-L" + os.path.join(ROOT, "lumahdrv_amd", "lib"), "-lluma_hip", "-llumahip",
                    "-Wl,-rpath," + os.path.join(ROOT, "lumahdrv_amd", "lib")], check=True)
    return exe
