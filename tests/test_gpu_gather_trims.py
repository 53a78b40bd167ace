"""Two trims of the gather-class kernels of rife-v4.6, against what they computed before - the bytes must not move.

  k_flow_cascade (csrc/flow_cascade.h): a thread forms the horizontal half of the interpolation once per cell row its four pixels touch.  tap 6 (the cascade on b
  injected flows) against tap 4 (k_flow_update after every injected flow), b = 2 and 3, byte for byte, with the taps and the injected flows of
  test_gpu_flow_cascade.py, at the sizes where the row groups differ: the smallest frame, whose two tiles hold one clamped row group each, a frame with a padded last
  tile row, many tiles along one axis only, a width that is no multiple of the 64-pixel tile, a ragged frame.

  stem_rs_kernel (csrc/stem_rs.h): all four stem-1 waves finish the output row, each the half of the S16 entries whose partial sums it kept.  The first S16
  tensor of block 3 (tap 7) against the oracle's blob with the comparison and the bars of test_gpu_s16_ends.py::test_block_stems_match_oracle - the test
  itself, called on this file's sizes: a second strip of one column, strips of 31, 31, 2 and of 31 x 3 + 3 columns, workgroups whose range crosses a strip
  change.  Tap 7 serves 8-bit frames only, and the depth changes nothing in the kernel but the unpacking of the frame dwords, so stem_rs_kernel<0, 10> is held
  at the same sizes through tap 5 - block 3's input carried through both stems by one-hot weights - against tap 0 (k_assemble<1, 10>, which test_gpu_deep.py
  holds to the oracle bit for bit) with that file's bar for the kernel: 2^-21 relative, twice the f16-subnormal floor.  Tap 5 drives output channels 0 .. 23 of
  stem 1 only: the output block n = 0, that is waves 0 and 2 with their hand-over, finish and 16-byte stores, and with one-hot weights one of the two K partial
  sums of a channel is zero.  Waves 1 and 3 and a sum of two non-zero chunks are held by the 8-bit oracle test above alone."""
import numpy as np
import pytest

import deep_ref
import test_gpu_s16_ends as s16e
from tools import gen_frames

from test_gpu_flow_cascade import engines, injected_flows      # noqa: F401  (engines: the module fixture of the cascade's own tests)
from test_gpu_s16_ends import stems                            # noqa: F401  (the engines, the oracle and the graph executor of the stem tests)

pytestmark = pytest.mark.gpu

# (w, h): 32x32 one tile column of two tiles, each with one clamped row group and three inner ones; 64x48 -> 64x64 padded, four tile rows;
# 32x512 / 512x32 many tiles on one axis, clamps at the first and last tile only; 96x80 width no multiple of the tile; 333x241 ragged, padded to 352x256
CASCADE_SIZES = [(32, 32), (64, 48), (32, 512), (512, 32), (96, 80), (333, 241)]


@pytest.mark.parametrize("w,h", CASCADE_SIZES)
@pytest.mark.parametrize("b", [2, 3])
def test_cascade_with_shared_row_lerps_writes_the_sequential_updates(engines, w, h, b):
    _, gt, _, _ = engines
    a, c = gen_frames.noise_pair(w, h, w + h)
    inj = injected_flows(w, h, 900 + w + b, b)
    assert all(f[4].std() > 0.5 for f in inj), "the mask channel is constant"
    want = gt.v4_tap(a, c, 0.5, 4, b, inj)
    got = gt.v4_tap(a, c, 0.5, 6, b, inj)
    hp, wp = (h + 31) // 32 * 32, (w + 31) // 32 * 32
    assert got.shape == want.shape == (5, hp, wp)
    assert np.abs(want[:4]).max() > 64, "injected flows too small: F stays within 64 pixels"
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "%d of %d floats differ, first at %s" % (
        int((got != want).sum()), want.size, np.argwhere(got.view(np.uint32) != want.view(np.uint32))[0])


# (w, h): 128x32 Wq = 32, a second strip of one column, Hq = 8; 256x64 strips of 31, 31, 2 columns; 384x96 31 x 3 + 3; 640x360 workgroup ranges across strips
STEM_RS_SIZES = [(128, 32), (256, 64), (384, 96), (640, 360)]


@pytest.mark.parametrize("w,h", STEM_RS_SIZES)
@pytest.mark.parametrize("kind", ["smooth", "noise"])
def test_stem_rs_with_four_finishing_waves_matches_the_oracle(stems, w, h, kind):
    s16e.test_block_stems_match_oracle(stems, (3, w, h, kind, "rs"))


@pytest.mark.parametrize("w,h", STEM_RS_SIZES)
def test_stem_rs_at_depth_10_carries_the_block_input(stems, w, h):
    g = stems["rs"]
    a, c = deep_ref.deep_pair(w, h, w + h, amp=512)
    inj = injected_flows(w, h, 300 + w, 3)
    want = g.v4_tap(a, c, 0.4, 0, 3, inj)
    got = g.v4_tap(a, c, 0.4, 5, 3, inj)
    assert want.shape == got.shape == (12, (h + 31) // 32 * 32, (w + 31) // 32 * 32) and np.abs(want[:6]).max() > 0.5
    err = np.abs(got - want) - (6e-7 * np.abs(want) + 2.4e-7)
    assert err.max() <= 0, "stem_rs_kernel<0, 10>: worst excess %g at %s" % (float(err.max()), np.unravel_index(int(err.argmax()), err.shape))
