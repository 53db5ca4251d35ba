"""bench.py's own contract: a plain run times the headline only, --full adds the rest, --dump-outputs writes what the last
timed step computed (float32, at most 64 MB, the same inputs run to run)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _bench(args, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True,
                       timeout=timeout, env={k: v for k, v in os.environ.items()
                                             if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")})
    line = next((ln for ln in reversed(r.stdout.splitlines()) if ln.startswith("{")), None)
    return r, (json.loads(line) if line else None)


def test_dump_outputs_caps_the_size_with_a_fixed_sample(tmp_path):
    big = torch.arange(20 * 2 ** 20, dtype=torch.float32)          # 80 MB alone: over the cap
    small = torch.arange(1000, dtype=torch.int32).reshape(10, 100)  # whole, as float32
    wide = torch.ones(3, dtype=torch.float64)                      # float64 stays float64
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small, "wide": wide})
    files = {d: {n: np.load(str(tmp_path / d / f"{n}.npy")) for n in ("big", "small", "wide")} for d in ("a", "b")}
    total = sum(os.path.getsize(str(tmp_path / "a" / f)) for f in os.listdir(str(tmp_path / "a")))
    assert total <= bench.DUMP_LIMIT_BYTES
    a, b = files["a"], files["b"]
    assert a["big"].dtype == np.float32 and 0 < a["big"].size < big.numel()
    assert np.array_equal(a["big"], b["big"])                     # the same sample every time
    assert np.all(np.diff(a["big"]) >= 0)                         # sorted element indices of the flattened array
    assert a["small"].dtype == np.float32 and np.array_equal(a["small"], small.numpy().astype(np.float32))
    assert a["wide"].dtype == np.float64


def test_strict_roofline_needs_full():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--strict-roofline"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 2 and "--full" in r.stderr


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_plain_run_times_the_headline_and_dumps_the_last_step(tmp_path):
    """Two plain runs at a reduced size: exactly --steps timed steps, the headline fields only, and the same radii and images
    (the forward composites every pixel in a fixed order) from the same inputs."""
    got = []
    for d in ("a", "b"):
        out = str(tmp_path / d)
        r, j = _bench(["--gpus", "1", "--steps", "7", "--warmup", "2", "--P", "20000", "--dump-outputs", out])
        assert r.returncode == 0 and j is not None, (r.stdout[-2000:], r.stderr[-3000:])
        assert j["steps"] == 7 and j["ms_per_step"] > 0 and j["unit"] == "Gaussians/s" and j["higher_is_better"] is True
        assert j["dtype"] == "f32" and abs(j["value"] - 20000 * 7 / (j["ms_per_step"] * 7e-3)) <= 1e-6 * j["value"]
        assert list(j["modes_ms_per_step"]) == ["graph"]
        assert "roofline" not in j and "cpu_baseline" not in j and j["long_run"] is None
        got.append({f[:-4]: np.load(os.path.join(out, f)) for f in os.listdir(out)})
    a, b = got
    names = {"color", "feat", "radii", "grad_means3D", "grad_scales", "grad_rotations", "grad_opacities", "grad_shs",
             "grad_language_feature"}
    assert set(a) == names and set(b) == names
    assert a["color"].shape == (3, 128, 128) and a["feat"].shape == (32, 128, 128) and a["radii"].shape == (20000,)
    assert a["grad_language_feature"].shape == (20000, 32)
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in a.values())
    assert (a["radii"] > 0).any() and np.abs(a["grad_means3D"]).max() > 0
    assert np.array_equal(a["radii"], b["radii"])
    assert np.allclose(a["color"], b["color"], rtol=0, atol=1e-6) and np.allclose(a["feat"], b["feat"], rtol=0, atol=1e-6)
    for n in names - {"color", "feat", "radii"}:
        assert np.allclose(a[n], b[n], rtol=1e-4, atol=1e-6 * np.abs(a[n]).max()), n  # (atomic sums: last bits may differ)
