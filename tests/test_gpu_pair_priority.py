"""K_pair's hot walker sets its wave priority from how far its walk has got
(pair1k.hip, CRLOT_PAIR_PRIO; at H = 256 on planar rows): once per trip of the main
loop (2U frames: 16 at H = 128, 8 at H = 256, 6 at H = 512) the priority becomes 3,
2, 1 or 0 as p = floor(64 done / M) passes 32, 52 and 60, M being the chunk length.
That is scheduling only, so the hot walker must still give the two-regime walker's
bits (pairing mode 2) at every walk length on either side of a boundary of the
policy: a single pair, one trip exactly, one trip plus a pair, K - 1 / K / K + 1
frames and trips for K = 8, 16, 32 (the cyclic codes that were measured) and 64,
chunk lengths that are no multiple of 64, and single-frame chunks."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 1024
S = 3


def bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy(), np.float32).view(np.uint32)


def trip_frames(h):
    nb = N // h
    ring = {1: 4, 2: 6, 4: 8}.get(nb, 16)  # PairRot<NB>::R hop slots, U = R / 2 pairs per trip
    return ring


def frame_counts(h):
    t = trip_frames(h)
    fc = {1, 2, 3, t, t + 1, t + 2}                       # a single pair, one trip, one trip plus a pair
    for k in (8, 16, 32, 64):
        fc |= {k - 1, k, k + 1}                          # K - 1, K, K + 1 frames: a step per frame
        fc |= {t * (k - 1), t * k, t * (k + 1) + 2}      # ... and a step per trip
    return sorted(fc)


def hot_and_two_regime(torch, plan, run):
    y_hot = run()
    assert plan.last_launch()["kernels"] == ["k_pair_hot", "k_pair_fix"]
    plan.set_frame_pairing(2)
    y_ref = run()
    assert plan.last_launch()["kernels"] != ["k_pair_hot", "k_pair_fix"]
    plan.set_frame_pairing(1)
    return y_hot, y_ref


@pytest.fixture(scope="module")
def signal(oracle):
    """One set of streams for every case (a case takes the first T samples)."""
    x = oracle.synth_streams(2 * S, max(h * frame_counts(h)[-1] for h in (128, 256, 512)), config_id=83)
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("h", [128, 256, 512])
def test_walk_lengths_around_every_policy_boundary(pkg, torch_cuda, signal, h):
    """One chunk per stream (chunks = 1, so M = F) at every frame count of
    frame_counts(h); T = F H - 3 keeps the last frame partly zero padding."""
    torch = torch_cuda
    plan = pkg.Plan(frame_size=N, hop_size=h)
    plan.set_chunks(1)
    for F in frame_counts(h):
        T = F * h - 3
        xd = torch.from_numpy(np.ascontiguousarray(signal[:S, :T])).cuda()
        y_hot, y_ref = hot_and_two_regime(torch, plan, lambda: plan.roundtrip(xd))
        assert plan.last_launch()["n_chunks"] == 1
        assert torch.equal(y_hot, y_ref), f"H={h} F={F}"


@pytest.mark.parametrize("h,F,chunks,m", [(128, 301, 3, 101), (256, 301, 3, 101), (512, 301, 3, 101),
                                          (256, 203, 7, 29), (256, 300, 1000, 1), (128, 300, 1000, 1),
                                          (512, 300, 1000, 1)])
def test_chunk_lengths_no_multiple_of_k(pkg, torch_cuda, signal, h, F, chunks, m):
    """Several chunks per stream whose length M is odd, prime or 1 (the chunk knob
    at F = 300 makes 300 single-frame chunks), so K done / M never lands on a step."""
    torch = torch_cuda
    plan = pkg.Plan(frame_size=N, hop_size=h)
    plan.set_chunks(chunks)
    xd = torch.from_numpy(np.ascontiguousarray(signal[:S, :F * h - 3])).cuda()
    y_hot, y_ref = hot_and_two_regime(torch, plan, lambda: plan.roundtrip(xd))
    assert plan.last_launch()["n_chunks"] == -(-F // m)
    assert torch.equal(y_hot, y_ref)


def test_interleaved_pair_of_channels(pkg, torch_cuda, signal):
    """C = 2 interleaved groups at H = 256: the strided walk (built without the
    policy) beside the planar one."""
    torch = torch_cuda
    h, F, C = 256, 137, 2
    T = F * h - 3
    plan = pkg.Plan(frame_size=N, hop_size=h)
    plan.set_chunks(3)
    x = signal[:S * C, :T].reshape(S, C, T)
    xi = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1))).cuda()  # (S, T, C)
    y_hot, y_ref = hot_and_two_regime(torch, plan, lambda: plan.roundtrip_interleaved(xi))
    assert torch.equal(y_hot, y_ref)


def test_nan_burst_in_a_middle_chunk(pkg, torch_cuda, signal):
    """A NaN burst in the middle chunk of three: the hot walker flags a cluster
    there and the fix-up walker redoes it, all under the policy.  NaN outputs
    compare by their bits."""
    torch = torch_cuda
    h, F = 256, 120
    T = F * h - 3
    x = np.array(signal[:S, :T])
    x[1, 60 * h + 17:60 * h + 22] = np.nan
    x[2, 61 * h] = 1e25
    plan = pkg.Plan(frame_size=N, hop_size=h)
    plan.set_chunks(3)
    xd = torch.from_numpy(x).cuda()
    y_hot, y_ref = hot_and_two_regime(torch, plan, lambda: plan.roundtrip(xd))
    assert plan.last_launch()["n_chunks"] == 3
    assert np.array_equal(bits(y_hot), bits(y_ref))
    assert torch.equal(y_hot[0], y_ref[0])
