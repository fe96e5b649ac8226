"""bench.py's stdout contract, checked without a GPU: the compact headline line built from a full measurement dict
(the committed detail of an earlier driver-shaped run) stays under the 6 KB cap, parses, and keeps the fields the
driver and the judge read (round 5's 25 KB line was not parsed by the driver)."""
import glob
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_compact_line_of_a_full_measurement_is_short_and_self_contained():
    bench = _bench()
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*", "bench_all_configs.json")))
    assert files
    for path in files:
        full = json.load(open(path))
        line = bench.compact(full)
        assert len(line) < bench.LINE_CAP and "\n" not in line, (path, len(line))
        out = json.loads(line)
        for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                  "dtype", "data", "config", "roofline"):
            assert k in out, (path, k)
        assert out["value"] == full["value"] and out["ms_per_step"] == full["ms_per_step"]
        assert out["roofline"]["frac"] == full["roofline"]["frac"] and out["roofline"]["bound"] in ("mfma", "hbm", "valu", "latency")
        assert "workload" in out["config"] and "model" not in out["config"]
        if "cpu_baseline" in full:
            assert out["cpu_baseline"]["value"] > 0 and out["cpu_baseline"]["cores"] == full["cpu_baseline"]["cores"]
        for c, o in out.get("other_configs", {}).items():
            assert set(o) <= {"value", "ms_per_step", "roofline", "fx_kernel_frac_of_independent_floor", "cpu_baseline",
                              "value_clips_trained", "error"}


def test_compact_line_sheds_optional_blocks_before_it_outgrows_the_cap():
    bench = _bench()
    full = json.load(open(sorted(glob.glob(os.path.join(ROOT, "profiles", "r*", "bench_all_configs.json")))[-1]))
    full["step_ms_per_rank"] = [[1.0, 2.0, 3.0]] * 2000            # an absurd world size
    out = json.loads(bench.compact(full))
    assert "step_ms_per_rank" in out["dropped_for_length"] and "roofline" in out and len(json.dumps(out)) < bench.LINE_CAP


def test_plain_run_is_the_default_and_the_options_reach_the_workers():
    """`--full` is off by default; `--steps` is the number of timed steps; the launcher hands `--full` to every worker
    and `--dump-outputs` (made absolute: the workers run in bench.py's directory) to the headline worker only."""
    bench = _bench()
    args = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2", "--dump-outputs", "out"])
    assert args.full is False and args.steps == 7 and args.warmup == 2
    assert args.dump_outputs == os.path.abspath("out")
    assert "--full" not in bench._worker_cmd(args, 3, args.steps)
    full = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2", "--full"])
    assert full.full is True and full.dump_outputs is None
    cmd = bench._worker_cmd(full, 2, 30)
    assert "--full" in cmd and cmd[cmd.index("--steps") + 1] == "30"


def test_dumped_outputs_are_float_sampled_the_same_way_and_capped(tmp_path):
    import numpy as np
    import torch
    bench = _bench()
    bench.torch = torch                     # (bench.py imports torch lazily in its worker)
    big = torch.randn(3, 1, bench.DUMP_SAMPLE)
    a, b = bench.dump_array(big, sample=True), bench.dump_array(big.clone(), sample=True)
    assert a.shape == (bench.DUMP_SAMPLE,) and a.dtype == np.float32 and np.array_equal(a, b)
    assert np.isin(a, big.numpy().reshape(-1)).all()
    small = torch.arange(10, dtype=torch.float64)
    assert bench.dump_array(small, sample=True).dtype == np.float64 and bench.dump_array(small).shape == (10,)
    assert bench.dump_array(torch.arange(4)).dtype == np.float32
    bench.dump_outputs(str(tmp_path / "d"), {"a": a, "loss": bench.dump_array(torch.tensor(0.25))})
    assert sorted(os.listdir(tmp_path / "d")) == ["a.npy", "loss.npy"]
    assert np.array_equal(np.load(tmp_path / "d" / "a.npy"), a) and float(np.load(tmp_path / "d" / "loss.npy")) == 0.25
    with pytest.raises(ValueError):
        bench.dump_outputs(str(tmp_path / "e"), {"x": np.zeros(bench.DUMP_CAP_BYTES // 4 + 1, np.float32)})
    assert not (tmp_path / "e").exists()
