"""The float64 reference (tests/f64_reference.py) against the oracle, on the CPU.

Proves the inputs of tests/test_gpu_local_accuracy.py fair before any GPU sees
them: at every shape and input of that file the oracle (the reference chain in
float32) is
  * within whole-stream rel-L2 1e-6 of the float64 restatement (measured
    1.0e-7 .. 1.6e-7),
  * within 4e-6 of it block by block, against the scale of the block's OWN
    frames (measured <= 4.2e-7, so the bar the GPU tests use has 10x headroom
    over the reference's own error), and
  * exactly +0 on every block whose covering frames are all gated to zero.
"""
import numpy as np
import pytest

import f64_reference as R

REL_L2 = 1e-6
LOCAL = 4e-6


def check(oracle, x, n, h, gain, mask, what):
    worst_l2 = worst_loc = 0.0
    for s in range(x.shape[0]):
        m = None if mask is None else R.stream_mask(mask, s)
        y = oracle.roundtrip_mask(x[s], n, h, bin_gain=gain, mask=m)
        y_ref, fs = R.roundtrip_f64(x[s], n, h, gain, m)
        assert y.shape == y_ref.shape, what
        l2 = np.linalg.norm(y - y_ref) / np.linalg.norm(y_ref)
        own = R.own_scale(fs, n, h)
        loc = R.local_err(y, y_ref, own, h)
        worst_l2, worst_loc = max(worst_l2, l2), max(worst_loc, loc)
        assert l2 <= REL_L2, f"{what} stream {s}: rel-L2 {l2:.3e}"
        assert loc <= LOCAL, f"{what} stream {s}: local_err(own) {loc:.3e}"
        assert R.silent_is_plus_zero(y, own, h), f"{what} stream {s}: a silent block is not +0"
    return worst_l2, worst_loc


@pytest.mark.parametrize("n,h", R.SHAPES)
def test_oracle_matches_f64_reference(oracle, n, h):
    x = R.make_streams(n, h)
    F = R.frame_count(x.shape[1], n, h)
    assert F >= 45 and oracle.frame_count(x.shape[1], n, h) == F
    rows = [check(oracle, x, n, h, None, None, f"{n}/{h} plain"),
            check(oracle, x, n, h, R.make_gain(n), None, f"{n}/{h} gain")]
    for v in R.GATE_VALUES:
        for kind in R.MASK_KINDS:
            rows.append(check(oracle, x, n, h, None, R.make_mask(n, F, v, kind), f"{n}/{h} {kind} v={v:g}"))
    print(f"{n}/{h}: rel-L2 <= {max(r[0] for r in rows):.2e}, local_err(own) <= {max(r[1] for r in rows):.2e}")


@pytest.mark.parametrize("n,h", [(512, 128), (1024, 512), (882, 441), (960, 240)])
def test_gates_open_silent_blocks(n, h):
    """The inputs do contain silent blocks (the exact-zero assertion is not vacuous):
    a zero gate silences blocks of the gated streams, leading silence those of s2."""
    x = R.make_streams(n, h)
    F = R.frame_count(x.shape[1], n, h)
    m = R.make_mask(n, F, 0.0, "per_stream")
    for s, want in ((0, True), (1, False), (2, True), (3, True)):
        _, fs = R.roundtrip_f64(x[s], n, h, None, m[s])
        assert (R.silent_blocks(R.own_scale(fs, n, h)).size > 0) == want, s
    # a gate that only attenuates silences nothing on a plain stream
    _, fs = R.roundtrip_f64(x[3], n, h, None, R.make_mask(n, F, 2.0 ** -24, "shared"))
    assert R.silent_blocks(R.own_scale(fs, n, h)).size == 0


def test_drop_framing_and_metric():
    """DROP framing against the oracle, and the metric on a hand-made case."""
    n, h = 512, 128
    x = R.make_streams(n, h)[0]
    y = R.O.roundtrip_ex(x, n, h, mode=R.DROP)
    y_ref, fs = R.roundtrip_f64(x, n, h, mode=R.DROP)
    assert y.shape == y_ref.shape and fs.size == (x.size - n) // h + 1
    assert np.linalg.norm(y - y_ref) / np.linalg.norm(y_ref) <= REL_L2
    fs = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 4.0, 1.0, 2.0])
    assert R.own_scale(fs, 4, 2).tolist() == [0, 0, 0, 0, 0, 4, 4, 2]       # nb = 2
    assert R.pair_scale(fs, 4, 2).tolist() == [0, 0, 0, 0, 4, 4, 4, 2]      # mate 5 of 4; 6 ^ 1 = 7
    assert R.silent_blocks(R.own_scale(fs, 4, 2)).tolist() == [0, 1, 2, 3, 4]
    y0 = np.zeros(16)
    y1 = y0.copy()
    y1[11] = 2.0                                                             # block 5, scale 4
    y1[1] = 9.0                                                              # a silent block: not in local_err
    assert R.local_err(y1, y0, R.own_scale(fs, 4, 2), 2) == 0.5
    assert not R.silent_is_plus_zero(y1, R.own_scale(fs, 4, 2), 2)
    assert not R.silent_is_plus_zero(-y0, R.own_scale(fs, 4, 2), 2)          # -0 is not +0
    assert R.silent_is_plus_zero(y0, R.own_scale(fs, 4, 2), 2)
