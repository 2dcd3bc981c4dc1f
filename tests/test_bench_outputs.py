"""bench.py's lean default run and --dump-outputs: the plain line holds what the headline needs, --full adds the rest, and
the dumped arrays are the last timed step's outputs, the same from run to run, within their size budget."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_KEYS = ("settled_ms_per_step", "roofline", "kernels", "host_call_ms", "cpu_baseline", "entropy_stage", "with_scaled_copy")


def _files(d):
    return {f[:-len(".npy")]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_options_parse():
    a = bench.parse(["--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    a = bench.parse(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])


def test_dump_keeps_the_budget_and_the_sample_fixed(tmp_path):
    """Arrays larger than their share become a seeded sample (the same positions every time); small ones are written
    whole; float64 stays float64, everything else is float32."""
    rng = np.random.default_rng(3)
    big = rng.standard_normal(1 << 24)                                    # 128 MiB of float64
    bins = rng.integers(0, 256, 1 << 24, dtype=np.uint8)
    small = rng.standard_normal(1000).astype(np.float32)
    named = [("reconstruction", big), ("bin_index", bins), ("dc", small), ("info", np.array([1.5, 2.0]))]
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), named)
    a, b = _files(tmp_path / "a"), _files(tmp_path / "b")
    assert sorted(a) == ["bin_index", "dc", "info", "reconstruction"]
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert sum(os.path.getsize(tmp_path / "a" / (f + ".npy")) for f in a) <= 64 << 20
    assert a["reconstruction"].dtype == np.float64 and a["bin_index"].dtype == np.float32 and a["dc"].dtype == np.float32
    assert np.array_equal(a["dc"], small) and np.array_equal(a["info"], [1.5, 2.0])
    assert 0 < a["reconstruction"].size < big.size and np.isin(a["reconstruction"], big).all()
    assert np.array_equal(a["bin_index"], np.round(a["bin_index"])) and a["bin_index"].max() <= 255


def _bench(*args, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--n", "128", "--steps", "3", "--warmup", "1"]
                       + list(args), capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_and_full_lines_and_dumped_outputs(tmp_path):
    """A plain run reports the headline only; --full adds the secondary figures.  Both dump the same outputs, and those are
    bit for bit the oracle's streams and reconstruction of the same input (2^21 elements: every array fits whole)."""
    from oracle import oracle as O
    from tests import workloads as W
    plain = _bench("--dump-outputs", str(tmp_path / "plain"))
    full = _bench("--full", "--no-cpu-baseline", "--no-entropy-stage", "--dump-outputs", str(tmp_path / "full"))
    for line in (plain, full):
        assert all(k in line for k in HEADLINE_KEYS) and line["steps"] == 3 and line["warmup"] == 1
        assert line["ms_per_step"] > 0 and line["value"] > 0 and line["dtype"] == "f64" and line["higher_is_better"] is True
    assert not any(k in plain for k in FULL_KEYS)
    assert all(k in full for k in ("settled_ms_per_step", "roofline", "kernels", "with_scaled_copy"))

    p, f = _files(tmp_path / "plain"), _files(tmp_path / "full")
    assert sorted(p) == sorted(f) == ["ac_exact", "bin_index", "dc", "info", "reconstruction"]
    assert all(np.array_equal(p[k], f[k]) for k in p)
    x = W.c3(128, seed=512)
    c = O.compress(x, 1e-3, O.EC, O.FAST)
    assert p["info"][0] == c.sf and p["info"][4] == c.cnt
    assert np.array_equal(p["bin_index"], c.bin_index.astype(np.float32))
    assert np.array_equal(p["dc"].view(np.uint32), c.dc.view(np.uint32))
    assert np.array_equal(p["ac_exact"].view(np.uint32), c.ac_exact.view(np.uint32))
    assert np.array_equal(p["reconstruction"].view(np.uint64), O.decompress(c, O.FAST).view(np.uint64))
