"""Builds a yardstick program of tests/cpp (tests/cpp/<name>.cpp -> tests/cpp/<name>.bin) against the in-tree library, once per session.
san=True is the variant the sanitizer tests run: a stand-alone program with its own main, built with -fsanitize=address,undefined into
tests/cpp/<name>_san.bin and run directly, never loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "orb_slam3_v1.0_amd", "csrc")
CPP = os.path.join(ROOT, "tests", "cpp")

_built = {}


def build(name, san=False, opt="-O2"):
    out = os.path.join(CPP, name + ("_san.bin" if san else ".bin"))
    if out in _built:  # once per session
        return out
    _built[out] = 1
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if san else [opt]
    subprocess.check_call(["g++"] + flags + ["-std=c++17", "-Wall", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                                             os.path.join(CPP, name + ".cpp"), "-o", out, "-L", CSRC, "-lorbfe",
                                             "-Wl,-rpath," + CSRC, "-Wl,-rpath,/opt/rocm/lib"])
    return out
