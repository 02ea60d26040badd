"""Oracle references for slices of a long stream.

The oracle runs at a few Msamples/s, so a test of a 2^27-sample stream cannot
run it over the whole stream.  It does not have to.  The reference chain has
finite memory: an output sample depends on the ceil(N/H) frames that cover it
and on the norm table entry at its position modulo the ring length.  So for a
slice start `a` that is a multiple of oracle.ring_len(n, h) (itself a multiple of
H at every shape used here; both are required),

    oracle.roundtrip(x[a:a+L])  ==  oracle.roundtrip(x)[a:a+L]     bit for bit

once ceil(N/H) - 1 blocks of H samples are skipped at the head of the slice (the
frames that start before `a` are missing there) and ceil(N/H) blocks at its tail
when the slice ends before the stream does (the slice's last frames are zero
padded where the stream goes on).  A slice that starts at 0 keeps the stream's
head, a slice that runs to the end keeps its tail: the last partial frame and
DROP framing are then the stream's own.  A start that is not ring aligned
reads another phase of the norm table and matches nowhere in general;
check_start refuses it.  tests/test_extent_reference.py asserts all of this.

stft rows have no such memory: row k is the transform of x[kH : kH+N], so any
slice start that is a multiple of H serves (stft_rows).
"""
from typing import Callable, List, NamedTuple, Tuple

import numpy as np


class Slice(NamedTuple):
    name: str
    a: int  # input samples [a, b) of the stream
    b: int


def blocks(n: int, h: int) -> int:
    return -(-n // h)


def margins(n: int, h: int, head_blocks: int = -1) -> Tuple[int, int]:
    """(head, tail) samples to skip in a slice's output: ceil(N/H) - 1 blocks at
    the head (head_blocks overrides the count), ceil(N/H) at the tail."""
    cb = blocks(n, h)
    return (cb - 1 if head_blocks < 0 else head_blocks) * h, cb * h


def check_start(a: int, n: int, h: int, ring: int):
    if a < 0 or a % ring != 0 or a % h != 0:
        raise ValueError(f"slice start {a} is not a multiple of the ring length {ring} (and of H = {h}): "
                         "its reference would not be the stream's")


def min_span(n: int, h: int, ring: int) -> int:
    """The shortest slice plan_slices accepts: room for a ring-aligned start on
    either side of T/2 and for at least one checked block between the margins."""
    return 2 * ring + (2 * blocks(n, h) + 1) * h + n


def plan_slices(T: int, n: int, h: int, ring: int, span: int) -> List[Slice]:
    """The head slice [0, span), one ring-aligned slice of `span` samples that
    straddles T/2, and a ring-aligned tail slice of at least `span` samples that
    runs to T (each clipped to the stream)."""
    if span < min_span(n, h, ring):
        raise ValueError(f"span {span} < {min_span(n, h, ring)}")
    a_mid = max(0, T // 2 - span // 2) // ring * ring
    a_tail = max(0, T - span) // ring * ring
    out = [Slice("head", 0, min(T, span)), Slice("mid", a_mid, min(T, a_mid + span)), Slice("tail", a_tail, T)]
    for sl in out:
        check_start(sl.a, n, h, ring)
    assert out[1].a <= T // 2 < out[1].b or T <= span
    return out


def valid_range(sl: Slice, T: int, out_len: int, n: int, h: int, head_blocks: int = -1) -> Tuple[int, int]:
    """[lo, hi) in stream coordinates where a slice's out_len output samples are
    the stream's own."""
    head, tail = margins(n, h, head_blocks)
    lo = sl.a + (0 if sl.a == 0 else head)
    hi = sl.a + out_len - (0 if sl.b >= T else tail)
    return lo, max(lo, hi)


def roundtrip_slice(run: Callable, fetch: Callable, sl: Slice, T: int, n: int, h: int, ring: int,
                    head_blocks: int = -1):
    """Reference for one slice.  fetch(a, b) returns x[a:b] as float32 numpy;
    run(x_slice, k0) returns the oracle's round trip of the slice, k0 = a / H being
    the stream's frame index of the slice's first frame (for a per-frame mask).
    Returns (lo, hi, ref): ref is the stream's output [lo, hi)."""
    check_start(sl.a, n, h, ring)
    ys = np.asarray(run(np.ascontiguousarray(fetch(sl.a, sl.b), np.float32), sl.a // h))
    lo, hi = valid_range(sl, T, ys.size, n, h, head_blocks)
    return lo, hi, ys[lo - sl.a:hi - sl.a]


def roundtrip_slices(run: Callable, fetch: Callable, T: int, n: int, h: int, ring: int, span: int,
                     head_blocks: int = -1):
    """(slice, lo, hi, ref) for the head, middle and tail slices of a stream of T samples."""
    for sl in plan_slices(T, n, h, ring, span):
        lo, hi, ref = roundtrip_slice(run, fetch, sl, T, n, h, ring, head_blocks)
        yield sl, lo, hi, ref


def stft_rows(spec_of: Callable, fetch: Callable, T: int, n: int, h: int, a: int, count: int):
    """Reference spectra of frames k0 = a / H ... of a stream: spec_of(x_slice)
    returns the oracle's (F, N/2+1) spectra of a slice.  Only rows whose frame
    lies inside the slice, or whose slice ends where the stream does, are the
    stream's.  Returns (k0, rows)."""
    if a < 0 or a % h != 0:
        raise ValueError(f"stft slice start {a} is not a multiple of H = {h}")
    b = min(T, a + (count - 1) * h + n)
    rows = np.asarray(spec_of(np.ascontiguousarray(fetch(a, b), np.float32)))
    keep = rows.shape[0] if b >= T else min(rows.shape[0], (b - a - n) // h + 1)
    return a // h, rows[:max(0, min(keep, count))]
