"""The row groups of k_flow_cascade (csrc/flow_cascade_geom.h) on the host: which cell rows the four pixels of a thread share.

A thread owns one column of its wave's four rows and forms the horizontal half of the interpolation once per cell row the rows touch; which pair of them a pixel
row blends is a constant per row and level for every row group away from up_coeff's vertical clamps (group_inner), and the kernel reads the cell rows from LDS
without a bounds check.  tests/sanitize/flow_cascade_rows_main.cpp includes the same header and, for every padded height 32 .. 4096 (step 32), every level and
every row group, restates the scheme on one column of cell values: each row's cell rows and weights must be up_coeff's (restated there in its float form), the
touched cell rows inside what the tile stages, and every row group but the image's first and last must take the constant pattern.  Built twice: plain, and with
ASan + UBSan as a stand-alone executable (the flags of csrc/Makefile's ../flow-cascade-rows-asan), where a cell row outside the staged rows is a heap overflow."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "sanitize", "flow_cascade_rows_main.cpp")
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


@pytest.mark.parametrize("flags", [["-O2"], SAN], ids=["plain", "asan-ubsan"])
def test_every_row_blends_the_cell_rows_of_up_coeff(tmp_path, flags):
    exe = str(tmp_path / "flow_cascade_rows")
    b = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + [SRC, "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    m = re.search(r"flow_cascade_rows: (\d+) checks, (\d+) mismatches", p.stdout.splitlines()[-1])
    assert m and int(m.group(1)) > 1000000 and int(m.group(2)) == 0, p.stdout[-500:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-2000:]


def test_the_makefile_builds_the_same_program_under_the_sanitizers():
    mk = open(os.path.join(ROOT, "rife-ncnn-vulkan_amd", "csrc", "Makefile")).read()
    rule = mk[mk.index("../flow-cascade-rows-asan:"):].split("\n", 2)
    assert "flow_cascade_rows_main.cpp" in rule[0] and "flow_cascade_geom.h" in rule[0]
    for f in SAN[2:]:
        assert f in rule[1], f
    assert "../flow-cascade-rows-asan" in mk[mk.index("\nsanitize:"):].split("\n", 2)[1]
