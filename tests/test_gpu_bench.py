"""bench.py on one device: a plain run with --dump-outputs at a small size, and the GPU-side
helpers: the N > 1 line's weak-scaling reference (a slab
stepped as a single domain before the communicator is attached, then re-initialised) leaves the
slab run exactly as a fresh slab would run it."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(REPO, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    m._imports()
    return m


def test_plain_run_dumps_the_last_step(gpu, tmp_path):
    """`bench.py --n 32 --steps 6 --warmup 3 --dump-outputs DIR` as a process: a plain line (no
    probe, secondary lattices or CPU baseline), and in DIR the fields and residual of a cavity
    stepped 9 times, bit for bit."""
    from lbm_amd import cases
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--n", "32", "--steps", "6",
                          "--warmup", "3", "--dump-outputs", str(tmp_path / "dump")],
                         capture_output=True, text=True, timeout=300, check=True)
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["steps"] == 6 and line["warmup"] == 3 and line["unit"] == "MLUPS" and line["dtype"] == "f32"
    assert line["value"] > 0 and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(32 ** 3 / (line["ms_per_step"] * 1e-3) / 1e6, rel=1e-2)
    assert "secondary" not in line and "cpu_baseline" not in line and line["roofline"]["stream_probe_gbs"] is None
    lat = cases.ldc_device(32, 32, 32)
    lat.step(9, history=False)
    state = lat.state()
    for k, ref in zip(("rho", "ux", "uy", "uz"), lat.macros()):
        got = np.load(tmp_path / "dump" / f"{k}.npy")
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    res = np.load(tmp_path / "dump" / "residual.npy")
    assert res.dtype == np.float64 and res.tolist() == [state["residual"], state["velsum"]]
    assert float(np.abs(np.load(tmp_path / "dump" / "ux.npy")).max()) > 0.0  # the lid has moved the fluid
    lat.close()


def test_single_domain_reference_then_slab_run(gpu):
    from lbm_amd import cases
    import lbm_amd
    b = _bench()
    a = cases.ldc_device(32, 32, 32, z_offset=32, nz_global=96)
    ms = b.single_domain_ms(a, 5)
    assert ms > 0.0
    a.init_ldc()  # what bench.py does before attaching
    a.attach_rccl(lbm_amd.rccl_unique_id(), 0, 1)
    fresh = cases.ldc_device(32, 32, 32, z_offset=32, nz_global=96)
    fresh.attach_rccl(lbm_amd.rccl_unique_id(), 0, 1)
    ha, hf = a.step(12), fresh.step(12)
    assert np.array_equal(ha.view(np.uint32), hf.view(np.uint32))
    for x, y in zip(a.macros(), fresh.macros()):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    a.close()
    fresh.close()
