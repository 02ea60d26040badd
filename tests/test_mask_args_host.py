"""Plan.set_spectral_mask's argument checks, without a device.

The kernels index the mask with (ld_stream, ld_frame) for the S x F frames of a
call and check nothing themselves, so a wrong dtype, a foreign device, a
broadcast stream dimension with a non-zero stride or a mask smaller than a later
call would all be out-of-bounds device reads.  The checks are pure functions over
plain tuples (pkg.mask_layout, pkg.check_mask_extent); no test here hands a bad
mask to the native call.
"""
import pytest

BINS = 513


def dense(*shape):
    st, acc = [], 1
    for d in reversed(shape):
        st.append(acc)
        acc *= d
    return tuple(shape), tuple(reversed(st))


def test_accepts_dense_masks(pkg):
    shape, st = dense(4, 50, BINS)
    assert pkg.mask_layout(shape, st, "float32", 0, 0, BINS) == (BINS, 50 * BINS, (4, 50))
    shape, st = dense(50, BINS)
    assert pkg.mask_layout(shape, st, "float32", 2, 2, BINS) == (BINS, 0, (None, 50))
    # padded rows keep their pitch
    assert pkg.mask_layout((4, 50, BINS), (50 * 520, 520, 1), "float32", 0, 0, BINS) == (520, 50 * 520, (4, 50))


def test_rejects_float64(pkg):
    shape, st = dense(4, 50, BINS)
    with pytest.raises(ValueError, match="float32"):
        pkg.mask_layout(shape, st, "float64", 0, 0, BINS)


def test_rejects_float16(pkg):
    shape, st = dense(50, BINS)
    with pytest.raises(ValueError, match="float32"):
        pkg.mask_layout(shape, st, "float16", 0, 0, BINS)


def test_rejects_wrong_device(pkg):
    shape, st = dense(50, BINS)
    with pytest.raises(ValueError, match="device"):
        pkg.mask_layout(shape, st, "float32", 1, 0, BINS)
    with pytest.raises(ValueError, match="device"):  # a host tensor
        pkg.mask_layout(shape, st, "float32", None, 0, BINS)


def test_rejects_bad_rows(pkg):
    with pytest.raises(ValueError):
        pkg.mask_layout((50, BINS - 1), (BINS - 1, 1), "float32", 0, 0, BINS)
    with pytest.raises(ValueError):
        pkg.mask_layout((50, BINS), (2 * BINS, 2), "float32", 0, 0, BINS)
    with pytest.raises(ValueError):
        pkg.mask_layout((BINS,), (1,), "float32", 0, 0, BINS)


def test_broadcast_stream_dimension_has_stride_zero(pkg):
    """(1, F, bins) serves every stream: ld_stream 0 whatever stride the size-1
    dimension reports, and no stream count to check later calls against."""
    shape, st = dense(1, 50, BINS)
    assert pkg.mask_layout(shape, st, "float32", 0, 0, BINS) == (BINS, 0, (None, 50))
    assert pkg.mask_layout(shape, (12345, BINS, 1), "float32", 0, 0, BINS) == (BINS, 0, (None, 50))
    pkg.check_mask_extent((None, 50), 64, 50)
    # an expanded view (stride 0 over S streams) is a broadcast too
    assert pkg.mask_layout((4, 50, BINS), (0, BINS, 1), "float32", 0, 0, BINS) == (BINS, 0, (4, 50))


def test_frames_too_short(pkg):
    pkg.check_mask_extent((4, 50), 4, 50)
    pkg.check_mask_extent(None, 4, 10 ** 6)  # no mask stored
    with pytest.raises(ValueError, match="50 frames.*51"):
        pkg.check_mask_extent((4, 50), 4, 51, "roundtrip")
    with pytest.raises(ValueError, match="frames"):
        pkg.check_mask_extent((None, 50), 1, 51)


def test_streams_too_short(pkg):
    pkg.check_mask_extent((4, 50), 3, 50)
    with pytest.raises(ValueError, match="4 streams.*5"):
        pkg.check_mask_extent((4, 50), 5, 50, "istft_ola")


class _HostPlan:
    """Plan's Python side with the size queries answered on the host."""

    def __new__(cls, pkg, n, h, extent):
        p = object.__new__(pkg.Plan)
        p._h = None
        p.frame_size, p.hop_size = n, h
        p._mask, p._mask_extent = object(), extent
        p.frame_count = lambda T: -(-T // h)
        p.output_length = lambda T: -(-T // h) * h
        return p


def test_interleaved_counts_every_channel(pkg):
    """roundtrip_interleaved reads G * C streams of mask rows: a mask of G streams is
    refused before the native call (the plan here has no native handle to call)."""
    import torch
    G, Cc, T, n, h = 2, 3, 5000, 1024, 256
    F = -(-T // h)
    x = torch.zeros((G, T, Cc))
    with pytest.raises(ValueError, match=f"{G} streams.*{G * Cc}"):
        _HostPlan(pkg, n, h, (G, F)).roundtrip_interleaved(x)
    with pytest.raises(ValueError, match="frames"):
        _HostPlan(pkg, n, h, (G * Cc, F - 1)).roundtrip_interleaved(x)
    pkg.check_mask_extent((G * Cc, F), G * Cc, F)
