"""crlot_spectrogram's staged form over more streams than one workspace slice holds
(the sibling of the other composites' *_in_two_slices tests; helpers from
test_gpu_features.py)."""
import pytest

from test_gpu_features import make_plan

pytestmark = pytest.mark.gpu


def test_spectrogram_in_two_slices(pkg, torch_cuda):
    """4096 / 1024 (no feature walker above N = 1024, no frame-pair feature kernel at
    4096), zero padding, S = 130, T = 131 072: F = 128; per stream 128 rows x 4098 floats
    x 4 bytes = 2 098 176 bytes; 268 435 456 // 2 098 176 = 127 streams per slice, so
    slices of 127 and 3 streams.  Equal, bit for bit, to the same call on sub-batches
    that are one slice each, the seam at stream 127 included."""
    torch = torch_cuda
    n, h, S, T = 4096, 1024, 130, 131072
    plan = make_plan(pkg, n, h)
    W = pkg.mel_filterbank(6, n, 16000.0)
    f = pkg.Features(plan, weights=W, log=pkg.FEAT_DB, floor=1e-10)
    x = torch.randn((S, T), device="cuda", generator=torch.Generator(device="cuda").manual_seed(13))
    x[:, 555::7000] += 30.0
    F = plan.frame_count(T)
    assert F == 128 and (1 << 28) // (F * (n + 2) * 4) == 127
    want = torch.cat([f.spectrogram(x[a:b]) for a, b in ((0, 64), (64, 128), (128, 130))])
    got = f.spectrogram(x)
    torch.cuda.synchronize()
    rec = plan.last_launch()
    assert got.shape == (S, F, 6) and bool(torch.isfinite(got).all())
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    # the record lists both slices' launches: one workgroup of k_feat_step per four
    # frame rows, 127 x 128 rows in the first slice and 3 x 128 in the last
    steps = [g for k, g in zip(rec["kernels"], rec["grid"]) if k == "k_feat_step"]
    assert rec["kernels"][-1] == "k_feat_step" and steps == [127 * F // 4, 3 * F // 4], rec
    f.close()
    plan.close()
