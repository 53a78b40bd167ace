#!/bin/bash
# ASan + UBSan and TSan job for the HOST side (csrc/main.cpp, rife.cpp, jpeg_codec.h, the PNG band writer); no GPU needed: the engine behind the C-ABI is
# tests/sanitize/stub_engine.cpp (+ stub_engine_deep.cpp / stub_engine_yuv.cpp for the 10-bit, RGBA and 4:2:0 entry points).  Writes a log to stdout; exit code != 0 if any sanitizer reported.
#   tools/sanitize_run.sh > profiles/r5/sanitize.txt
set -u
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd $ROOT
make -s -C rife-ncnn-vulkan_amd/csrc sanitize || exit 2
ASAN=$ROOT/rife-ncnn-vulkan_amd/rife-hip-asan
TSAN=$ROOT/rife-ncnn-vulkan_amd/rife-hip-tsan
export ASAN_OPTIONS=exitcode=99:detect_leaks=1:abort_on_error=0
export UBSAN_OPTIONS=halt_on_error=1:exitcode=98:print_stacktrace=1
export TSAN_OPTIONS=halt_on_error=1:exitcode=66:second_deadlock_stack=1
FAIL=0
echo "== $(g++ --version | head -1); $(date -u +%Y-%m-%dT%H:%MZ); $(nproc) cores"
echo "== 1. decoder corpus of tests/test_cli.py (truncated / bit-flipped / crafted png, jpg baseline + progressive, bmp, pnm; PNG colour types; codec round trips) through the ASan + UBSan binary"
echo "   (a sanitizer report exits 99 / 98, which the tests' 'returncode in (0, 1)' assertions reject)"
RIFE_HIP_BIN=$ASAN python -m pytest tests/test_cli.py -q -m "not gpu" -k "cpp_cli" 2>&1 | tail -4
[ ${PIPESTATUS[0]} -eq 0 ] || FAIL=1
echo "== 1b. the 10-bit codecs (--transcode10: 16-bit png, ppm with maxval 1023 / 65535, truncated and crafted files) of tests/test_cli_deep.py through the same binary"
RIFE_HIP_BIN=$ASAN python -m pytest tests/test_cli_deep.py -q -m "not gpu" -k "cpp_cli" 2>&1 | tail -4
[ ${PIPESTATUS[0]} -eq 0 ] || FAIL=1
echo "== 1c. the RGBA codecs (--transcode -a: png colour types 4 / 6, tRNS, 16-bit, webp, 32-bit bmp, truncated and crafted files) of tests/test_cli_alpha.py through the same binary"
RIFE_HIP_BIN=$ASAN python -m pytest tests/test_cli_alpha.py -q -m "not gpu" -k "cpp_cli" 2>&1 | tail -4
[ ${PIPESTATUS[0]} -eq 0 ] || FAIL=1
echo "== 1d. the YUV4MPEG2 reader and writer (headers, rate fraction, schedule, in-order output from 4 save threads, truncated / malformed files, flags out of scope) of tests/test_cli_yuv.py through the same binary"
RIFE_HIP_BIN=$ASAN python -m pytest tests/test_cli_yuv.py -q -m "not gpu" -k "cpp_cli" 2>&1 | tail -4
[ ${PIPESTATUS[0]} -eq 0 ] || FAIL=1
T=$(mktemp -d)
python - $T <<'PY'
import sys, os
sys.path.insert(0, os.getcwd())
import numpy as np
from PIL import Image
from tools import gen_frames
t = sys.argv[1]
for sub in ("png", "jpg", "ppm"):
    os.makedirs(os.path.join(t, "in_" + sub))
for i in range(7):
    a = gen_frames.smooth_pair(333, 241, 40 + i)[i & 1]           # ragged size: PNG filter rows / JPEG edge MCUs
    Image.fromarray(a).save(os.path.join(t, "in_png", "%03d.png" % i))
    Image.fromarray(a).save(os.path.join(t, "in_jpg", "%03d.jpg" % i), quality=92, progressive=bool(i & 1))
    Image.fromarray(a).save(os.path.join(t, "in_ppm", "%03d.ppm" % i))
big = gen_frames.smooth_pair(1920, 1080, 9)                       # large enough for the band-parallel PNG writer (1 MB bands)
os.makedirs(os.path.join(t, "in_big"))
for i in range(3):
    Image.fromarray(big[i & 1]).save(os.path.join(t, "in_big", "%03d.png" % i))
PY
run() {   # name binary args...
    local name=$1; shift
    "$@" > $T/log.txt 2>&1
    local rc=$?
    local nout=$(ls $T/out 2>/dev/null | wc -l)
    echo "   $name: rc $rc, $nout files"
    if [ $rc -ne 0 ]; then FAIL=1; tail -30 $T/log.txt; fi
}
echo "== 2. directory mode under TSan: 3-stage pipeline, two replicas (-g 0,1 and -g 0,0), several load / proc / save threads; outputs must equal the 1-replica run"
for fmt in png jpg ppm; do
    rm -rf $T/out $T/ref; mkdir -p $T/out
    run "tsan $fmt -g 0 -j 1:2:2" $TSAN -i $T/in_$fmt -o $T/out -m rife-v4.6 -n 19 -f %08d.$fmt -g 0 -j 1:2:2
    mv $T/out $T/ref; mkdir -p $T/out
    run "tsan $fmt -g 0,1 -j 3:2,3:4" $TSAN -i $T/in_$fmt -o $T/out -m rife-v4.6 -n 19 -f %08d.$fmt -g 0,1 -j 3:2,3:4
    diff -rq $T/ref $T/out > /dev/null && echo "      == the 1-replica outputs" || { echo "      DIFFERS from the 1-replica outputs"; FAIL=1; }
    rm -rf $T/out; mkdir -p $T/out
    run "tsan $fmt -g 0,0 -j 2:1,2:3" $TSAN -i $T/in_$fmt -o $T/out -m rife-v4.6 -n 19 -f %08d.$fmt -g 0,0 -j 2:1,2:3
    diff -rq $T/ref $T/out > /dev/null && echo "      == the 1-replica outputs" || { echo "      DIFFERS from the 1-replica outputs"; FAIL=1; }
done
echo "== 3. the same under ASan + UBSan (heap / bounds / UB in the pipeline, the frame cache and the codecs), and the band-parallel PNG writer at 1920x1080 under both"
for fmt in png jpg ppm; do
    rm -rf $T/out; mkdir -p $T/out
    run "asan $fmt -g 0,1 -j 3:2,3:4" $ASAN -i $T/in_$fmt -o $T/out -m rife-v4.6 -n 19 -f %08d.$fmt -g 0,1 -j 3:2,3:4
done
rm -rf $T/out; mkdir -p $T/out
run "asan 1080p png (band writer)" $ASAN -i $T/in_big -o $T/out -m rife-v4.6 -n 5 -g 0 -j 1:2:2
rm -rf $T/out; mkdir -p $T/out
run "tsan 1080p png (band writer)" $TSAN -i $T/in_big -o $T/out -m rife-v4.6 -n 5 -g 0 -j 2:2:2
python - $T <<'PY'
import sys, os, numpy as np
from PIL import Image
t = sys.argv[1]
a = np.asarray(Image.open(os.path.join(t, "in_big", "000.png")).convert("RGB")); b = np.asarray(Image.open(os.path.join(t, "in_big", "001.png")).convert("RGB"))
o = np.asarray(Image.open(os.path.join(t, "out", sorted(os.listdir(os.path.join(t, "out")))[1])).convert("RGB"))
want = (np.float32(0.4) * a.astype(np.float32) + np.float32(0.6) * b.astype(np.float32) + np.float32(0.5)).astype(np.uint8)      # -n 5 over 3 frames: output 2 = frames 0, 1 at timestep 0.6
print("   band-written 1080p PNG decodes (PIL) to the stub's blend of its inputs:", bool(np.abs(o.astype(int) - want.astype(int)).max() <= 1))
PY
echo "== 3b. -b 10 (16-bit png in, 16-bit png / maxval-1023 ppm out; u16 frames through upload_px / process_frames of the stub) under both"
python - $T <<'PY'
import sys, os
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import deep_ref
from test_cli_deep import write_png, png_value
t = sys.argv[1]
os.makedirs(os.path.join(t, "in_deep"))
for i in range(5):
    write_png(os.path.join(t, "in_deep", "%03d.png" % i), png_value(deep_ref.deep_pair(333, 241, 70 + i)[i & 1]), 16)
PY
for fmt in png ppm; do
    rm -rf $T/out; mkdir -p $T/out
    run "asan -b 10 $fmt -g 0,1 -j 3:2,3:4" $ASAN -i $T/in_deep -o $T/out -m rife-v4.6 -n 13 -b 10 -f %08d.$fmt -g 0,1 -j 3:2,3:4
    rm -rf $T/out; mkdir -p $T/out
    run "tsan -b 10 $fmt -g 0,0 -j 2:1,2:3" $TSAN -i $T/in_deep -o $T/out -m rife-v4.6 -n 13 -b 10 -f %08d.$fmt -g 0,0 -j 2:1,2:3
done
echo "== 3c. -a (RGBA png in, RGBA png / webp out; four-byte frames through upload_px / process_frames of the stub) under both"
python - $T <<'PY'
import sys, os
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
from PIL import Image
import alpha_ref
t = sys.argv[1]
os.makedirs(os.path.join(t, "in_alpha"))
for i in range(5):
    Image.fromarray(alpha_ref.rgba_pair(333, 241, 80 + i, "smooth")[i & 1], "RGBA").save(os.path.join(t, "in_alpha", "%03d.png" % i))
PY
for fmt in png webp; do
    rm -rf $T/out; mkdir -p $T/out
    run "asan -a $fmt -g 0,1 -j 3:2,3:4" $ASAN -i $T/in_alpha -o $T/out -m rife-v4.6 -n 13 -a -f %08d.$fmt -g 0,1 -j 3:2,3:4
    rm -rf $T/out; mkdir -p $T/out
    run "tsan -a $fmt -g 0,0 -j 2:1,2:3" $TSAN -i $T/in_alpha -o $T/out -m rife-v4.6 -n 13 -a -f %08d.$fmt -g 0,0 -j 2:1,2:3
done
python - $T <<'PY'
import sys, os, numpy as np
from PIL import Image
t = sys.argv[1]
names = sorted(os.listdir(os.path.join(t, "out")))
im = Image.open(os.path.join(t, "out", names[0]))
print("   -a output is RGBA:", im.mode == "RGBA", im.size)
PY
echo "== 3d. video mode (.y4m in, .y4m out; 4:2:0 frames through upload_px / process_frames of the stub, the in-order writer behind several save threads) under both"
python - $T <<'PY'
import sys, os
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import yuv_ref as yr
from test_cli_yuv import write_y4m, random_frames
t = sys.argv[1]
write_y4m(os.path.join(t, "odd.y4m"), "YUV4MPEG2 W333 H241 F30000:1001 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED", random_frames(9, 333, 241, yr.PIX_I420, 1))
write_y4m(os.path.join(t, "p10.y4m"), "YUV4MPEG2 W333 H241 F25:1 Ip C420p10", random_frames(5, 333, 241, yr.PIX_I420P10, 2))
PY
for v in odd p10; do
    run "asan $v.y4m -g 0 -j 1:1:1" $ASAN -i $T/$v.y4m -o $T/ref.y4m -m rife-v4.6 -n 23 -g 0 -j 1:1:1
    run "asan $v.y4m -g 0,1 -j 3:2,3:4" $ASAN -i $T/$v.y4m -o $T/out.y4m -m rife-v4.6 -n 23 -g 0,1 -j 3:2,3:4
    cmp -s $T/ref.y4m $T/out.y4m && echo "      == the 1-thread file" || { echo "      Y4M DIFFERS from the 1-thread file"; FAIL=1; }
    run "tsan $v.y4m -g 0,1 -j 3:2,3:4" $TSAN -i $T/$v.y4m -o $T/out.y4m -m rife-v4.6 -n 23 -g 0,1 -j 3:2,3:4
    cmp -s $T/ref.y4m $T/out.y4m && echo "      == the 1-thread file" || { echo "      Y4M DIFFERS from the 1-thread file"; FAIL=1; }
    $TSAN -i $T/$v.y4m -o - -m rife-v4.6 -n 23 -g 0,0 -j 2:1,2:3 > $T/out.y4m 2> $T/log.txt; rc=$?
    echo "   tsan $v.y4m -o - -g 0,0 -j 2:1,2:3: rc $rc"; [ $rc -ne 0 ] && { FAIL=1; tail -30 $T/log.txt; }
    cmp -s $T/ref.y4m $T/out.y4m && echo "      == the 1-thread file" || { echo "      Y4M DIFFERS from the 1-thread file"; FAIL=1; }
done
for bad in "YUV4MPEG2 W8 H6 F25:1 C422" "YUV4MPEG2 W8 H6 F25:1 It C420" "YUV4MPEG2 W0 H6 F25:1 C420" "YUV4MPEG2 W99999999 H99999999 F25:1 C420" "YUV4MPEG2 W8 H6 F25:1 C420 FRAME"; do
    { printf '%s\n' "$bad"; head -c 100 /dev/zero; } > $T/bad.y4m
    for B in $ASAN $TSAN; do
        $B -i $T/bad.y4m -o $T/bad_out.y4m -m rife-v4.6 > $T/log.txt 2>&1; rc=$?
        [ $rc -eq 1 ] || { echo "   $(basename $B) malformed header '$bad': rc $rc (a refusal is 1)"; FAIL=1; tail -20 $T/log.txt; }
    done
done
head -c 300 $T/odd.y4m > $T/bad.y4m
for B in $ASAN $TSAN; do
    $B -i $T/bad.y4m -o $T/bad_out.y4m -m rife-v4.6 > $T/log.txt 2>&1; rc=$?
    [ $rc -eq 1 ] && grep -q truncated $T/log.txt || { echo "   $(basename $B) truncated file: rc $rc"; FAIL=1; tail -20 $T/log.txt; }
done
echo "   malformed headers and a truncated file: refused with exit status 1 by both binaries"
echo "== 4. single-pair mode, error paths (missing file, size mismatch, bad extension) under ASan + UBSan"
rm -rf $T/out; mkdir -p $T/out
run "asan pair" $ASAN -0 $T/in_png/000.png -1 $T/in_png/001.png -o $T/out/o.png -m rife-v4.6 -s 0.3
$ASAN -0 $T/in_png/000.png -1 $T/nothing.png -o $T/out/o2.png -m rife-v4.6 > $T/log.txt 2>&1; rc=$?; echo "   asan missing input: rc $rc (sanitizer exit codes are 99 / 98)"; [ $rc -ge 98 ] && [ $rc -le 99 ] && FAIL=1
$ASAN -0 $T/in_png/000.png -1 $T/in_big/000.png -o $T/out/o3.png -m rife-v4.6 > $T/log.txt 2>&1; rc=$?; echo "   asan size mismatch: rc $rc"; [ $rc -ge 98 ] && [ $rc -le 99 ] && FAIL=1
echo "== 4b. flow scale (-d 2 through RIFE::set_flow_scale of the stub; refusals of -d 3 and of another family end before any engine exists) under both"
for B in $ASAN $TSAN; do
    run "$(basename $B) pair -d 2" $B -0 $T/in_png/000.png -1 $T/in_png/001.png -o $T/out/d2.png -m rife-v4.6 -d 2
    $B -0 $T/in_png/000.png -1 $T/in_png/001.png -o $T/out/d3.png -m rife-v4.6 -d 3 > $T/log.txt 2>&1; rc=$?
    [ $rc -eq 255 ] && [ ! -e $T/out/d3.png ] || { echo "   $(basename $B) -d 3: rc $rc (a refusal is 255 and writes nothing)"; FAIL=1; tail -20 $T/log.txt; }
    $B -0 $T/in_png/000.png -1 $T/in_png/001.png -o $T/out/d23.png -m rife-v2.3 -d 2 > $T/log.txt 2>&1; rc=$?
    [ $rc -eq 255 ] && [ ! -e $T/out/d23.png ] || { echo "   $(basename $B) -d 2 -m rife-v2.3: rc $rc (a refusal is 255 and writes nothing)"; FAIL=1; tail -20 $T/log.txt; }
done
echo "== 4c. precision (-p fast through RIFE::set_precision of the stub; refusals of an unknown word and of another family end before any engine exists) under both"
for B in $ASAN $TSAN; do
    run "$(basename $B) pair -p fast" $B -0 $T/in_png/000.png -1 $T/in_png/001.png -o $T/out/pf.png -m rife-v4.6 -p fast
    $B -0 $T/in_png/000.png -1 $T/in_png/001.png -o $T/out/pb.png -m rife-v4.6 -p bogus > $T/log.txt 2>&1; rc=$?
    [ $rc -eq 255 ] && [ ! -e $T/out/pb.png ] || { echo "   $(basename $B) -p bogus: rc $rc (a refusal is 255 and writes nothing)"; FAIL=1; tail -20 $T/log.txt; }
    $B -0 $T/in_png/000.png -1 $T/in_png/001.png -o $T/out/p23.png -m rife-v2.3 -p fast > $T/log.txt 2>&1; rc=$?
    [ $rc -eq 255 ] && [ ! -e $T/out/p23.png ] || { echo "   $(basename $B) -p fast -m rife-v2.3: rc $rc (a refusal is 255 and writes nothing)"; FAIL=1; tail -20 $T/log.txt; }
done
echo "== 5. rife_hip_image_check's rules (csrc/image_check.h, host only) over refusing and accepting descriptors, a program of its own under ASan + UBSan"
$ROOT/rife-ncnn-vulkan_amd/image-check-asan > $T/log.txt 2>&1; rc=$?
echo "   image-check-asan: rc $rc, $(tail -1 $T/log.txt)"; [ $rc -ne 0 ] && { FAIL=1; tail -30 $T/log.txt; }
rm -rf $T
echo "== result: $([ $FAIL -eq 0 ] && echo CLEAN || echo FAILED)"
exit $FAIL
