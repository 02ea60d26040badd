"""GPU tests of the streaming convolver (include/crlot_dsp.h, "streaming convolution"):
every output block equal, bit for bit, to crlot_convolve over the concatenated input
with frame pairing off, at every E instantiation, past two wraps of the ring and through
the flush; the bits independent of the route, the prefetch mode, the channel count, a
channel's position and the layout; NULL blocks; reset; memory containment; accuracy
against np.convolve in float64 under the bar the float32 CPU oracle sets.

Inputs (tests/convolve_reference.py make_streams / make_filter): white noise, a silent
block-aligned stretch per stream and a 2^12 level step; decaying-noise filters.
"""
import functools

import numpy as np
import pytest

import convolve_reference as CR

pytestmark = pytest.mark.gpu


def same_bits(torch, a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


_convs = {}


def conv_for(pkg, B, P, nf=1):
    """A convolver of P partitions (K ends 7 taps into the last one; P = 1: 3 short of B)."""
    key = (B, P, nf)
    if key not in _convs:
        K = (P - 1) * B + 7 if P > 1 else B - 3
        h = CR.make_filter(nf, K, seed=P)
        conv = pkg.Convolver(h, block=B)
        assert conv.partitions == P
        _convs[key] = (conv, h)
    return _convs[key]


@functools.lru_cache(maxsize=None)
def streams(S, T, B, seed=0):
    x = CR.make_streams(S, T, B, seed)
    x.setflags(write=False)
    return x


def offline(torch, conv, x):
    """conv.convolve(x) with frame pairing off on the engine plan: (S, T + K - 1)."""
    plan = conv.plan
    plan.set_frame_pairing(False)
    try:
        y = conv.convolve(x)
        torch.cuda.synchronize()
    finally:
        plan.set_frame_pairing(True)
    return y


def run_stream(torch, sc, x, n_hops, prefetch=False):
    """Push x (C, T), the last block zero-padded, then NULL blocks up to n_hops.  (C, n_hops B)."""
    C, T = x.shape
    B = sc.block
    F_in = -(-T // B)
    xp = torch.zeros((C, F_in * B), device="cuda")
    xp[:, :T] = x
    blocks = []
    for j in range(n_hops):
        blk = xp[:, j * B:(j + 1) * B].contiguous() if j < F_in else None
        if blk is not None and sc.interleaved:
            blk = blk.t().contiguous()
        out = sc.push(blk)
        if prefetch:
            sc.prefetch()
        blocks.append(out.t() if sc.interleaved else out)
    torch.cuda.synchronize()
    return torch.cat(blocks, dim=1)


def frames_for(B, P, T):
    K = (P - 1) * B + 7 if P > 1 else B - 3
    return T + K - 1, -(-(T + K - 1) // B)


# ------------------------------------------------------------------ 1. equal to offline, bit for bit
# every E instantiation (B / 64 = 2, 4, 8, 16); P = 1 (route 1 always), 2, 3, 5 and 37
EQ_CASES = [(128, 1), (128, 2), (128, 3), (128, 5), (128, 37), (256, 4), (512, 3), (1024, 2)]


@pytest.mark.parametrize("B,P", EQ_CASES)
def test_blocks_equal_offline_convolve_bit_for_bit(pkg, torch_cuda, B, P):
    """Channels 1, 3, 5, 9 (a dead wave, a second and a third workgroup), n_filters in
    {1, 2, channels}; T = F_in B - 5 with F_in = max(12, 2P + 3): the ring wraps twice;
    NULL blocks to F_out + 2, the two extra blocks +0 in bits.  One case carries a NaN,
    an Inf and a 1e-38 sample."""
    torch = torch_cuda
    F_in = max(12, 2 * P + 3)
    T = F_in * B - 5
    L, F_out = frames_for(B, P, T)
    for C, nf in ((1, 1), (3, 2), (5, 5), (9, 2)):
        conv, _ = conv_for(pkg, B, P, nf)
        xh = np.array(streams(C, T, B, seed=B + P))
        if C == 3:
            xh[0, 5], xh[1, B + 2], xh[2, 3 * B + 9] = np.nan, np.inf, np.float32(1e-38)
            xh[1, 2 * B:3 * B] = np.float32(-0.0)
        x = torch.from_numpy(xh).cuda()
        want = offline(torch, conv, x)
        sc = pkg.StreamConvolver(conv, C)
        assert sc.state_bytes == 4 * C * (P * (2 * B + 2) + 2 * B + 2 + B)
        got = run_stream(torch, sc, x, F_out + 2)
        assert sc.hops == F_out + 2
        assert same_bits(torch, got[:, :L], want), (C, nf)
        assert int(got[:, F_out * B:].contiguous().view(torch.int32).abs().max()) == 0, (C, nf)
        assert bool(torch.any(got[:, (F_out - 1) * B:F_out * B] != 0))
        rec = sc.last_launch()
        # the library's choice: one launch at P = 1, and at P = 2 up to B = 512
        assert rec["route"] == (1 if P == 1 or (P == 2 and B <= 512) else 2) and rec["head_name"] == "k_sconv_head"
        sc.close()


# ------------------------------------------------------------------ 2. routes and prefetch
@pytest.mark.parametrize("B,P", [(128, 2), (128, 5), (128, 37), (512, 3)])
def test_routes_and_prefetch_modes_give_the_same_bits(pkg, torch_cuda, B, P):
    torch = torch_cuda
    C = 5
    conv, _ = conv_for(pkg, B, P, 2)
    T = max(12, 2 * P + 3) * B - 5
    L, F_out = frames_for(B, P, T)
    x = torch.from_numpy(np.array(streams(C, T, B, seed=P))).cuda()
    want = offline(torch, conv, x)
    head_grid, tail_grid = -(-C // 4), C * -(-(B + 1) // 64)
    outs = {}
    for name, route, auto, prefetch in (("one launch", 1, True, False), ("automatic", 2, True, False),
                                        ("manual", 2, False, True), ("manual, never called", 2, False, False)):
        sc = pkg.StreamConvolver(conv, C)
        sc.set_route(route)
        sc.set_prefetch(auto)
        outs[name] = run_stream(torch, sc, x, F_out, prefetch=prefetch)
        rec = sc.last_launch()
        assert rec["route"] == route and rec["head_name"] == "k_sconv_head" and rec["head_grid"] == head_grid, name
        if route == 1:
            assert rec["tail_name"] is None and rec["tail_grid"] == 0 and rec["tail_pending"] == 0
        else:
            # (never called: the tail of the last hop is still pending; every earlier one ran in front of the next head)
            assert rec["tail_name"] == "k_sconv_tail" and rec["tail_grid"] == tail_grid, name
            assert rec["tail_pending"] == (1 if name == "manual, never called" else 0), name
        if name == "manual, never called":
            sc.prefetch()
            assert sc.last_launch()["tail_pending"] == 0
            sc.prefetch()   # nothing pending: nothing enqueued
        # the route is fixed once a hop has run, until reset
        with pytest.raises(RuntimeError):
            sc.set_route(1)
        torch.cuda.synchronize()
        sc.reset()
        sc.set_route(0)
        assert sc.hops == 0 and sc.last_launch()["head_name"] is None
        sc.close()
    for name, got in outs.items():
        assert same_bits(torch, got[:, :L], want), name


def test_manual_prefetch_record_before_the_first_tail(pkg, torch_cuda):
    torch = torch_cuda
    B, P, C = 128, 3, 2
    conv, _ = conv_for(pkg, B, P, 1)
    sc = pkg.StreamConvolver(conv, C)
    sc.set_prefetch(False)
    sc.prefetch()                                    # nothing pending yet
    assert sc.last_launch()["tail_name"] is None
    sc.push(torch.zeros((C, B), device="cuda"))
    rec = sc.last_launch()
    assert rec["tail_pending"] == 1 and rec["tail_name"] is None and rec["tail_grid"] == 0
    sc.prefetch()
    rec = sc.last_launch()
    assert rec["tail_pending"] == 0 and rec["tail_name"] == "k_sconv_tail" and rec["tail_grid"] == C * 3
    torch.cuda.synchronize()
    sc.close()


# ------------------------------------------------------------------ 3. independence
@pytest.mark.parametrize("B,P", [(128, 5), (256, 4)])
def test_channels_alone_and_interleaved(pkg, torch_cuda, B, P):
    torch = torch_cuda
    C = 5
    conv, h = conv_for(pkg, B, P, 2)
    T = 9 * B - 5
    _, F_out = frames_for(B, P, T)
    x = torch.from_numpy(np.array(streams(C, T, B, seed=3))).cuda()
    sc = pkg.StreamConvolver(conv, C)
    base = run_stream(torch, sc, x, F_out)
    sc.close()
    inter = pkg.StreamConvolver(conv, C, interleaved=True)
    assert same_bits(torch, run_stream(torch, inter, x, F_out), base)
    inter.close()
    # channel c of the batch uses filter c mod 2: alone, through a convolver of that filter
    singles = [pkg.Convolver(h[q], block=B) for q in range(2)]
    for c in range(C):
        one = pkg.StreamConvolver(singles[c % 2], 1)
        assert same_bits(torch, run_stream(torch, one, x[c:c + 1], F_out)[0], base[c]), c
        one.close()
    for s in singles:
        s.close()


# ------------------------------------------------------------------ 4. NULL blocks and gaps
def test_null_block_mid_stream(pkg, torch_cuda):
    torch = torch_cuda
    B, P, C = 128, 3, 3
    conv, _ = conv_for(pkg, B, P, 2)
    F_in = 10
    xh = np.array(streams(C, F_in * B, B, seed=11))
    xh[:, 4 * B:5 * B] = 0.0
    x = torch.from_numpy(xh).cuda()
    L, F_out = frames_for(B, P, F_in * B)
    want = offline(torch, conv, x)
    a, b = pkg.StreamConvolver(conv, C), pkg.StreamConvolver(conv, C)
    ya, yb = [], []
    for j in range(F_out):
        blk = x[:, j * B:(j + 1) * B].contiguous() if j < F_in else None
        ya.append(a.push(None if j == 4 else blk))                                  # NULL for the gap
        yb.append(b.push(torch.zeros((C, B), device="cuda") if blk is None else blk))  # explicit zeros throughout
    torch.cuda.synchronize()
    ya, yb = torch.cat(ya, dim=1), torch.cat(yb, dim=1)
    assert same_bits(torch, ya, yb)
    assert same_bits(torch, ya[:, :L], want)
    a.close()
    b.close()


# ------------------------------------------------------------------ 5. reset
def test_reset(pkg, torch_cuda):
    torch = torch_cuda
    B, P, C = 256, 4, 3
    conv, _ = conv_for(pkg, B, P, 1)
    T = 7 * B
    _, F_out = frames_for(B, P, T)
    x = torch.from_numpy(np.array(streams(C, T, B, seed=5))).cuda() * 64.0
    sc = pkg.StreamConvolver(conv, C)
    first = run_stream(torch, sc, x, 7)          # stop mid-tail: ring, partial chain and carry are loud
    assert bool(torch.any(first != 0))
    sc.reset()
    assert sc.hops == 0
    silent = run_stream(torch, sc, torch.zeros((C, B), device="cuda"), P + 2)
    assert int(silent.contiguous().view(torch.int32).abs().max()) == 0          # +0, bit for bit
    sc.reset()
    again = run_stream(torch, sc, x, F_out)
    fresh = pkg.StreamConvolver(conv, C)
    assert same_bits(torch, again, run_stream(torch, fresh, x, F_out))
    assert same_bits(torch, again[:, :7 * B], first)
    sc.close()
    fresh.close()


# ------------------------------------------------------------------ 6. containment
@pytest.mark.parametrize("interleaved", [False, True])
def test_containment_and_overlap(pkg, torch_cuda, interleaved):
    torch = torch_cuda
    B, P, C = 128, 3, 5
    conv, _ = conv_for(pkg, B, P, 2)
    sc = pkg.StreamConvolver(conv, C, interleaved=interleaved)
    shape = (B, C) if interleaved else (C, B)
    n = B * C
    buf = torch.full((3 * n,), 77.0, device="cuda")
    out = buf[n:2 * n].view(shape)
    blk = torch.from_numpy(np.array(streams(C, B, B, seed=2))).cuda()
    blk = blk.t().contiguous() if interleaved else blk
    keep = blk.clone()
    for _ in range(P + 1):
        sc.push(blk, out=out)
    torch.cuda.synchronize()
    assert bool(torch.all(buf[:n] == 77.0)) and bool(torch.all(buf[2 * n:] == 77.0))
    assert bool(torch.all(out != 77.0)) and same_bits(torch, blk, keep)
    # overlapping in / out: refused by the Python front and by the library
    with pytest.raises(ValueError):
        sc.push(out, out=out)
    L_ = pkg.lib()
    hops = sc.hops
    assert L_.crlot_stream_convolve_hop(sc._h, buf.data_ptr() + 4, buf.data_ptr() + 4 * (n - 1), None) == pkg.EINVAL
    assert "overlap" in L_.crlot_last_error().decode() and sc.hops == hops
    assert L_.crlot_stream_convolve_hop(sc._h, buf.data_ptr(), None, None) == pkg.EINVAL
    sc.close()


# ------------------------------------------------------------------ 7. accuracy, directly
@pytest.mark.parametrize("case", CR.ACCURACY_CASES, ids=lambda c: "B%d_T%d_K%d_S%d_nf%d" % c)
def test_stream_accuracy_against_float64(pkg, oracle, torch_cuda, case, capsys):
    """Per channel rel-L2 and max-abs over max|y64| against np.convolve in float64; the bar
    per metric is the larger of the project's 1e-6 / 4e-6 and 4x what the float32 CPU
    oracle reaches on the same input and metric (tests/test_gpu_convolve.py's rule)."""
    torch = torch_cuda
    B, T, K, S, nf = case
    x = streams(S, T, B)
    h = CR.make_filter(nf, K)
    conv = pkg.Convolver(h, block=B)
    y64 = CR.convolve_f64(x, h)
    ofig = CR.error_figures(CR.convolve_oracle_f32(oracle, x, h, B), y64)
    L = T + K - 1
    sc = pkg.StreamConvolver(conv, S)
    y = run_stream(torch, sc, torch.from_numpy(np.array(x)).cuda(), -(-L // B))[:, :L]
    dfig = CR.error_figures(y.cpu().numpy(), y64)
    with capsys.disabled():
        print("\nstream convolve accuracy", case, "device", " ".join("(%.2e, %.2e)" % f for f in dfig), "oracle",
              " ".join("(%.2e, %.2e)" % f for f in ofig))
    for (l2, peak), (ol2, opeak) in zip(dfig, ofig):
        bar_l2, bar_peak = CR.bars(ol2, opeak)
        assert l2 <= bar_l2 and peak <= bar_peak, (l2, peak, bar_l2, bar_peak)
    sc.close()
    conv.close()
