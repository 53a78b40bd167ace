"""The operand lane maps of the conv_rs / conv_rs2 consumer waves (csrc/rs_frag_geom.h) on the host.

The consumers issue v_mfma_f32_16x16x32_f16 and take every operand address from that header: pixel fragments from the LDS ring rows (plain image, no half
swap), weight fragments from conv_t64's weight image, the identity fragments of the skip connection, and the quads of the fp32 staging rows.
tests/sanitize/rs_frag_geom_main.cpp includes the same header and checks, over every lane, tap, chunk pair, plane, pixel half, channel half and output block:
offsets inside their arrays, every (pixel, channel) and (output channel, input channel) exactly once with the same k on both sides of the product, the weight
rows in channel order through s16_row_channel, no bank conflict in any ds_read_b128 / ds_write_b128 lane group, the one-hot identity, and the unit sequence.
Built twice: plain, and with ASan + UBSan as a stand-alone executable (the flags of csrc/Makefile's ../rs-frag-geom-asan), where an offset outside a ring row,
the image or a staged row is a heap overflow."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "sanitize", "rs_frag_geom_main.cpp")
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


@pytest.mark.parametrize("flags", [["-O2"], SAN], ids=["plain", "asan-ubsan"])
def test_every_operand_lane_map_of_the_consumers(tmp_path, flags):
    exe = str(tmp_path / "rs_frag_geom")
    b = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + [SRC, "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    m = re.search(r"rs_frag_geom: (\d+) checks, (\d+) wrong", p.stdout.splitlines()[-1])
    assert m and int(m.group(1)) > 50000 and int(m.group(2)) == 0, p.stdout[-500:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-2000:]


def test_the_makefile_builds_the_same_program_under_the_sanitizers():
    mk = open(os.path.join(ROOT, "rife-ncnn-vulkan_amd", "csrc", "Makefile")).read()
    rule = mk[mk.index("../rs-frag-geom-asan:"):].split("\n", 2)
    assert "rs_frag_geom_main.cpp" in rule[0] and "rs_frag_geom.h" in rule[0]
    for f in SAN[2:]:
        assert f in rule[1], f
    assert "../rs-frag-geom-asan" in mk[mk.index("\nsanitize:"):].split("\n", 2)[1]
