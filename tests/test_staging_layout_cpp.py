"""tests/cpp/staging_layout.cpp: the layout of a host-pointer call (csrc/staging.h) without a GPU.  The program includes staging.h alone,
is built stand-alone with -fsanitize=address,undefined (its own main, never loaded into Python) and run directly.  It takes blocks of
element sizes 1, 4, 8 and odd record sizes with counts 0, 1, 63, 64, 65 across the three phases -- also with no scratch, with no inputs,
with an input that is a result too, with scratch behind and between the results, and with inputs out of phase order (flagged) -- and checks the device offsets against a plain Carver, the
host addresses, the result mirror, that no two blocks share a byte, and the two sizes.  It then puts, "uploads", "downloads" and gets
every block in two heap buffers of exactly host_bytes() and device_bytes(): the sizes are exact, so an overrun is a sanitizer failure."""
import subprocess

import cpp_build


def test_staging_layout_under_sanitizers(built):
    exe = cpp_build.build("staging_layout", san=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = p.stdout.decode()
    print(out)
    assert p.returncode == 0, out
    assert "staging_layout: ok" in out and "FAIL" not in out, out
    for script in ("in+scratch+out", "no scratch", "no inputs", "inout", "scratch behind the results", "scratch between results", "nothing"):
        assert script + ":" in out, out
