"""bench.py's plain run and --dump-outputs: the line a plain run prints (the
timed steps only, `ms_per_step`, no strong phase, no CPU baseline) and the
arrays it writes -- the output buffer of the last timed step, whole when small,
else a fixed seeded sample of it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_sample_is_fixed_and_bounded(tmp_path):
    """Above DUMP_WHOLE_BYTES: DUMP_ROWS whole rows and DUMP_POINTS flat samples,
    drawn from DUMP_SEED and the shape alone, equal to the buffer at those
    indices, float32, the same on a second call."""
    import torch
    import bench as B
    S, L = 64, 70_000  # 17.9 MB of f32: just past the 16 MiB written whole
    assert S * L * 4 > B.DUMP_WHOLE_BYTES
    y = torch.from_numpy(np.random.default_rng(5).standard_normal((S, L)).astype(np.float32))
    files = B.dump_outputs(torch, y, str(tmp_path / "a"))
    assert sorted(files) == ["roundtrip_points.npy", "roundtrip_rows.npy"]
    rows, pts = (np.load(tmp_path / "a" / f) for f in ("roundtrip_rows.npy", "roundtrip_points.npy"))
    assert rows.dtype == pts.dtype == np.float32
    assert rows.shape == (B.DUMP_ROWS, L) and pts.shape == (B.DUMP_POINTS,)
    rng = np.random.default_rng(B.DUMP_SEED)
    ri = np.sort(rng.choice(S, size=B.DUMP_ROWS, replace=False))
    fi = np.sort(rng.integers(0, S * L, size=B.DUMP_POINTS, dtype=np.int64))
    assert len(set(ri.tolist())) == B.DUMP_ROWS
    yn = y.numpy()
    assert np.array_equal(rows, yn[ri]) and np.array_equal(pts, yn.reshape(-1)[fi])
    B.dump_outputs(torch, y, str(tmp_path / "b"))
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
    # the headline shape stays under the 64 MB a dump may take
    assert (B.DUMP_ROWS * B.T_LEN + B.DUMP_POINTS) * 4 + 256 <= 64e6


@pytest.mark.gpu
def test_plain_bench_times_its_steps_and_dumps_the_last_output(tmp_path, torch_cuda, pkg):
    torch = torch_cuda
    import bench as B
    S, steps = 8, 3
    out_dir = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
           "--streams", str(S), "--dump-outputs", str(out_dir)]
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["steps"] == steps and out["full"] is False
    assert out["strong_scaling"] is None and out["cpu_baseline"] is None
    assert out["unit"] == "Msamples/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    # value and ms_per_step are the same measurement (ms_per_step is rounded to 1e-4 ms)
    assert out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(S * B.T_LEN / out["ms_per_step"] / 1e3, rel=1e-2)
    # one step is S x T_LEN x 4 B = 15.4 MB of output: written whole
    assert out["dumped_outputs"]["files"] == {"roundtrip.npy": [S, B.T_LEN]}
    y = np.load(out_dir / "roundtrip.npy")
    assert y.dtype == np.float32 and y.shape == (S, B.T_LEN)
    dev = torch.device("cuda", 0)
    x = B.synth_device(torch, S, B.T_LEN, dev, 0xC0FFEE)  # rank 0's seed in bench.py
    plan = pkg.Plan(frame_size=B.N_FFT, hop_size=B.HOP)
    y1 = plan.roundtrip(x).cpu().numpy()
    assert np.array_equal(y.view(np.uint32), y1.view(np.uint32))
