"""The tile geometry of k_flow_cascade (csrc/flow_cascade_geom.h) on the host: which coarse flow cells a tile stages in LDS.

The kernel copies, per level, the cells between up_coeff's clamped index at the tile's first pixel and at its last pixel (+ 1); every pixel then reads its
cell pair from LDS without a bounds check.  tests/sanitize/flow_cascade_geom_main.cpp includes the same header and sweeps every padded frame size 32 .. 4096
(step 32) on both axes, the scales 8 / 4 / 2 and every tile origin: each pixel's (s0, s0 + 1) from up_coeff (restated there in its float form) inside the staged
range, the range inside [0, in - 1], and the records of a tile inside the kernel's LDS allocation.  Built twice: plain, and with ASan + UBSan as a stand-alone
executable (the flags of csrc/Makefile's ../flow-cascade-geom-asan), where an index outside the flow or outside an LDS row is a heap overflow."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "sanitize", "flow_cascade_geom_main.cpp")
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


@pytest.mark.parametrize("flags", [["-O2"], SAN], ids=["plain", "asan-ubsan"])
def test_every_pixel_reads_inside_the_staged_cells(tmp_path, flags):
    exe = str(tmp_path / "flow_cascade_geom")
    b = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + [SRC, "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    m = re.search(r"flow_cascade_geom: (\d+) checks, (\d+) wrong", p.stdout.splitlines()[-1])
    assert m and int(m.group(1)) > 1000000 and int(m.group(2)) == 0, p.stdout[-500:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-2000:]


def test_the_makefile_builds_the_same_program_under_the_sanitizers():
    mk = open(os.path.join(ROOT, "rife-ncnn-vulkan_amd", "csrc", "Makefile")).read()
    rule = mk[mk.index("../flow-cascade-geom-asan:"):].split("\n", 2)
    assert "flow_cascade_geom_main.cpp" in rule[0] and "flow_cascade_geom.h" in rule[0]
    for f in SAN[2:]:
        assert f in rule[1], f
    assert "../flow-cascade-geom-asan" in mk[mk.index("\nsanitize:"):].split("\n", 2)[1]
