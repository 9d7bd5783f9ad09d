"""bench.py's plain run and --dump-outputs: the plain line carries the headline fields and nothing that --full adds, --steps sets
the number of timed steps, and the dumped planes are what a direct call of the timed path computes on the same input -- finite
(the raster's interior), whole for a small raster, at the fixed sample for a larger one, and the same from two row-block ranks
as from one."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _bench(args, out_dir, ranks=1, timeout=240):
    bench = os.path.join(ROOT, "bench.py")
    env = dict(os.environ)
    if ranks == 1:
        cmd = [sys.executable, bench, "--gpus", "1"]
    else:
        with socket.socket() as so:
            so.bind(("127.0.0.1", 0))
            port = so.getsockname()[1]
        env.update(XDEM_BENCH_SHARE_GPU="1", MASTER_ADDR="127.0.0.1")
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks), "--master-addr",
               "127.0.0.1", "--master-port", str(port), bench, "--gpus", str(ranks)]
    p = subprocess.run(cmd + args + ["--dump-outputs", str(out_dir)], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def _direct(n):
    """The 11 planes of the timed path computed by one direct call on the raster bench.py synthesises."""
    sys.path.insert(0, ROOT)
    import bench
    from xdem_amd import terrain
    from xdem_amd.synth import fbm_torch

    dev = torch.device("cuda", 0)
    dem = fbm_torch(n, n, dev, seed=42, row0=0, total_rows=n)
    out = terrain.terrain_attributes_device(dem, bench.FULL, resolution=10.0, surface_fit="Florinsky", curv_method="geometric")
    torch.cuda.synchronize()
    return bench, out.cpu().numpy()


def _load(d, names):
    return {k: np.load(os.path.join(str(d), f"{k}.npy")) for k in names}


@pytest.mark.parametrize("n", [1000, 1100])
def test_plain_run_line_and_dumped_planes(tmp_path, n):
    res = _bench(["--steps", "4", "--warmup", "1", "--size", str(n)], tmp_path)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in res, k
    assert res["steps"] == 4 and res["n_gpus"] == 1 and res["unit"] == "Mpixels/s" and res["higher_is_better"] is True
    # (both figures come from the same wall-clock time of the 4 timed steps; the tolerance covers their rounding)
    assert res["ms_per_step"] > 0 and abs(res["value"] - n * n / (res["ms_per_step"] * 1e3)) <= 0.02 * res["value"] + 0.1
    for k in ("roofline", "secondary", "cpu_baseline", "end_to_end", "device_state"):   # --full only
        assert k not in res, k
    bench, want = _direct(n)
    got = _load(tmp_path, bench.FULL)
    assert sorted(os.listdir(str(tmp_path))) == sorted(f"{k}.npy" for k in bench.FULL)
    from xdem_amd.dist import halo_depth

    depth = halo_depth(bench.FULL, "Florinsky", 3)
    (rows, cols), shape = bench.dump_positions(n, depth)
    m = n - 2 * depth
    if m * m <= bench.DUMP_SAMPLES:
        assert shape == (m, m) and got["slope"].shape == (m, m)
    else:
        assert shape is None and got["slope"].shape == rows.shape and 0 < rows.size <= bench.DUMP_SAMPLES
    assert rows.min() >= depth and rows.max() < n - depth and cols.min() >= depth and cols.max() < n - depth
    assert sum(a.nbytes for a in got.values()) <= 64 * 2**20
    for i, k in enumerate(bench.FULL):
        assert got[k].dtype == np.float32 and np.isfinite(got[k]).all(), k
        assert np.array_equal(got[k].reshape(-1), want[i][rows, cols]), k


def test_dumped_sample_is_the_same_from_two_row_block_ranks(tmp_path):
    one, two = tmp_path / "one", tmp_path / "two"
    args = ["--steps", "2", "--warmup", "1", "--size", "1100"]
    _bench(args, one)
    res = _bench(args, two, ranks=2)
    assert res["n_gpus"] == 2 and "secondary" not in res
    names = sorted(os.listdir(str(one)))
    assert names == sorted(os.listdir(str(two))) and len(names) == 11
    for f in names:
        assert np.array_equal(np.load(os.path.join(str(one), f)), np.load(os.path.join(str(two), f))), f
