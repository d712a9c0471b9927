"""bench.py driver-contract smoke: runs on CPU, emits the JSON line."""
import json
import os
import subprocess
import sys


def _run_bench(*extra):
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    out = subprocess.run(
        [sys.executable, "bench.py", "--model", "llama-tiny",
         "--micro-batch", "1", "--seq-len", "64", *extra],
        cwd=repo, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
    return json.loads(line)


def test_bench_cpu_smoke():
    rec = _run_bench("--steps", "1", "--warmup", "0", "--grad-accum", "1")
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup",
                "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config"):
        assert key in rec, key
    assert rec["n_gpus"] == 1
    assert rec["unit"] == "tokens/s"
    assert rec["data"] == "synthetic"
    assert rec["value"] > 0
    assert rec["config"]["seq_len"] == 64


def test_bench_dump_outputs_and_full(tmp_path):
    """--dump-outputs writes float32/float64 arrays of the LAST timed step
    that are identical from run to run (the CPU path is deterministic);
    --steps really sets how many steps run; --full is accepted and reports
    the same headline fields."""
    import numpy as np
    names = ["loss.npy", "weights_norm.npy", "weights_sample.npy"]

    def run(tag, steps, warmup, *extra):
        d = tmp_path / tag
        rec = _run_bench("--steps", str(steps), "--warmup", str(warmup),
                         "--grad-accum", "2", "--dump-outputs", str(d),
                         *extra)
        assert sorted(os.listdir(d)) == names
        assert rec["steps"] == steps and rec["warmup"] == warmup
        assert rec["ms_per_step"] > 0
        return rec, {f: np.load(d / f) for f in names}

    rec_a, a = run("a", 2, 1)
    rec_b, b = run("b", 2, 1, "--full")
    _, c = run("c", 1, 2)     # same 3 steps in all, split differently
    _, d = run("d", 1, 1)     # one step fewer
    total = 0
    for f in names:
        want = np.float64 if f == "weights_norm.npy" else np.float32
        assert a[f].dtype == want, (f, a[f].dtype)
        assert np.isfinite(a[f]).all(), f
        total += a[f].nbytes
        # same arguments => same inputs => same outputs
        np.testing.assert_array_equal(a[f], b[f], err_msg=f)
        # the dump is of the last step run: warmup + steps decide it, so
        # 1+2 and 2+1 agree (a dump taken after warmup would not) ...
        np.testing.assert_array_equal(a[f], c[f], err_msg=f)
        # ... and one timed step fewer gives other losses and weights, so
        # --steps does drive the loop
        assert not np.array_equal(a[f], d[f]), f
    assert total <= 64 * 2 ** 20
    assert a["loss.npy"].shape == (2,)   # one per micro-step
    assert rec_a["metric"] == rec_b["metric"]
    assert rec_a["dtype"] == rec_b["dtype"]
    assert rec_a["unit"] == rec_b["unit"]
