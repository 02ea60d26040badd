"""The property tests/extent_reference.py rests on, asserted on the CPU.

For a ring-aligned slice start the oracle's round trip of the slice is the
stream's, bit for bit, inside a margin of ceil(N/H) blocks at both ends; the
head slice keeps the stream's head and the tail slice its tail (last partial
frame, DROP framing).  A start that is not ring aligned does not match and is
refused.  One FrameQueue plan (centred, reflect padding) at the head slice.
"""
import numpy as np
import pytest

import extent_reference as ER

# (N, H, boundary mode): the shapes test_gpu_extents.py takes references for
SHAPES = [(1024, 256, 0), (4096, 2048, 0), (4096, 1024, 0), (960, 240, 0), (480, 120, 1), (882, 441, 0),
          (1024, 300, 0), (1920, 480, 0)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def streams(oracle):
    """x and the whole-stream round trip of every shape, computed once."""
    out = {}
    for n, h, mode in SHAPES:
        ring = oracle.ring_len(n, h)
        T = 40 * ring + 37 * n + 13  # ragged: the last frame is partial
        x = oracle.synth(T, 0xE47 + n + h)
        out[(n, h, mode)] = (ring, T, x, oracle.roundtrip(x, n, h, mode=mode))
    return out


@pytest.mark.parametrize("n,h,mode", SHAPES)
def test_slices_are_the_streams_own(oracle, streams, n, h, mode):
    ring, T, x, y = streams[(n, h, mode)]
    assert ring % h == 0
    cb = ER.blocks(n, h)
    span = ER.min_span(n, h, ring) + 3 * n + 5
    seen = []
    for sl, lo, hi, ref in ER.roundtrip_slices(lambda xs, k0: oracle.roundtrip(xs, n, h, mode=mode),
                                               lambda a, b: x[a:b], T, n, h, ring, span, head_blocks=cb):
        assert sl.a % ring == 0 and hi - lo >= h, (sl, lo, hi)
        assert np.array_equal(bits(ref), bits(y[lo:hi])), (n, h, sl)
        seen.append((sl.name, lo, hi))
    (hn, hlo, hhi), (mn, mlo, mhi), (tn, tlo, thi) = seen
    assert (hn, mn, tn) == ("head", "mid", "tail")
    assert hlo == 0                      # the head slice keeps the stream's head
    assert thi == y.size                 # the tail slice its tail: last partial frame, DROP's shorter output
    assert mlo <= T // 2 < mhi and mlo > 0 and mhi < y.size and hhi < y.size


@pytest.mark.parametrize("n,h,mode", SHAPES)
def test_stated_margins_suffice(oracle, streams, n, h, mode):
    """ceil(N/H) - 1 blocks at the head of a slice, ceil(N/H) at its tail (the helper's defaults)."""
    ring, T, x, y = streams[(n, h, mode)]
    a = (T // 2) // ring * ring
    sl = ER.Slice("mid", a, a + 2 * ring + 3 * n + 5)
    lo, hi, ref = ER.roundtrip_slice(lambda xs, k0: oracle.roundtrip(xs, n, h, mode=mode), lambda p, q: x[p:q], sl, T,
                                     n, h, ring)
    assert lo == a + (ER.blocks(n, h) - 1) * h
    assert np.array_equal(bits(ref), bits(y[lo:hi])), (n, h)


@pytest.mark.parametrize("n,h,mode", SHAPES)
def test_unaligned_start_is_refused_and_would_not_match(oracle, streams, n, h, mode):
    ring, T, x, y = streams[(n, h, mode)]
    a = (T // 2) // ring * ring + h  # a multiple of H, not of the ring
    L = 2 * ring
    with pytest.raises(ValueError):
        ER.check_start(a, n, h, ring)
    with pytest.raises(ValueError):
        ER.roundtrip_slice(lambda xs, k0: oracle.roundtrip(xs, n, h, mode=mode), lambda p, q: x[p:q],
                           ER.Slice("bad", a, a + L), T, n, h, ring)
    with pytest.raises(ValueError):
        ER.check_start(ring + 1, n, h, ring)
    ys = oracle.roundtrip(x[a:a + L], n, h, mode=mode)
    head, tail = ER.margins(n, h, ER.blocks(n, h))
    assert not np.array_equal(bits(ys[head:ys.size - tail]), bits(y[a + head:a + ys.size - tail]))


@pytest.mark.parametrize("n,h,mode", SHAPES)
def test_masked_slices_follow_the_frame_index(oracle, streams, n, h, mode):
    """With a per-frame mask the slice takes the mask rows from its first frame's index on."""
    ring, T, x, _ = streams[(n, h, mode)]
    F = oracle.frame_count(T, n, h, mode)
    m = np.random.default_rng(n).uniform(0.25, 1.0, (F, n // 2 + 1)).astype(np.float32)
    y = oracle.roundtrip_mask(x, n, h, mask=m, mode=mode)
    span = ER.min_span(n, h, ring)
    for sl, lo, hi, ref in ER.roundtrip_slices(
            lambda xs, k0: oracle.roundtrip_mask(xs, n, h, mask=m[k0:k0 + oracle.frame_count(xs.size, n, h, mode)],
                                                 mode=mode),
            lambda a, b: x[a:b], T, n, h, ring, span):
        assert np.array_equal(bits(ref), bits(y[lo:hi])), (n, h, sl)


@pytest.mark.parametrize("n,h,mode", SHAPES)
def test_stft_rows_from_any_hop_multiple(oracle, streams, n, h, mode):
    ring, T, x, _ = streams[(n, h, mode)]
    _, spec = oracle.roundtrip_mask(x, n, h, mode=mode, want_spec=True)
    F = spec.shape[0]

    def spec_of(xs):
        return oracle.roundtrip_mask(xs, n, h, mode=mode, want_spec=True)[1]

    for a, count in ((0, 7), (7 * h, 9), ((F - 6) * h, 6), ((F // 2) * h + h, 5)):
        k0, rows = ER.stft_rows(spec_of, lambda p, q: x[p:q], T, n, h, a, count)
        assert k0 == a // h and rows.shape[0] == count, (a, rows.shape)
        assert np.array_equal(rows.view(np.float32).view(np.uint32),
                              spec[k0:k0 + count].view(np.float32).view(np.uint32)), (n, h, a)
    with pytest.raises(ValueError):
        ER.stft_rows(spec_of, lambda p, q: x[p:q], T, n, h, h + 1, 2)


def test_framequeue_head_slice(oracle):
    """FrameQueue framing, centred with reflect padding: the head slice keeps the
    stream's padded head; the slice's own reflected tail stays inside the margin."""
    n, h = 1024, 256
    ring = oracle.ring_len(n, h)
    T = 30 * ring + 777
    x = oracle.synth(T, 0xF0)
    kw = dict(mode=oracle.FRAMEQUEUE, center=True, pad_mode=oracle.PAD_REFLECT)
    y = oracle.roundtrip_ex(x, n, h, **kw)
    sl = ER.Slice("head", 0, ER.min_span(n, h, ring))
    lo, hi, ref = ER.roundtrip_slice(lambda xs, k0: oracle.roundtrip_ex(xs, n, h, **kw), lambda a, b: x[a:b], sl, T,
                                     n, h, ring, head_blocks=ER.blocks(n, h))
    assert lo == 0 and hi > sl.b - 2 * n
    assert np.array_equal(bits(ref), bits(y[lo:hi]))
