"""bench.py's plain run, ``--full`` and ``--dump-outputs``, on the CPU path (one process, no GPU).

A plain run times the headline steps only; ``--full`` adds the second batch point; ``--dump-outputs``
writes what the last timed step computed, identically from run to run and whether or not
``--full`` passes follow it.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--device", "cpu", "--model", "gpt-nano", "--seq", "64", "--batch", "4",
         "--vocab", "65", "--steps", "3", "--warmup", "1"]
NAMES = ("loss", "grad_norm", "params")


def _bench(args):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """(result line, dump dir) of: a plain run, the same run again, the same run under --full."""
    out = []
    for tag, more in (("a", []), ("b", []), ("full", ["--full", "--also-batch", "2"])):
        d = str(tmp_path_factory.mktemp(tag))
        out.append((_bench([*SMALL, *more, "--dump-outputs", d]), d))
    return out


def test_plain_run_times_the_headline_steps_only(runs):
    j, _ = runs[0]
    assert j["full"] is False and j["steps"] == 3 and j["warmup"] == 1
    assert j["ms_per_step"] > 0 and j["value"] > 0
    assert j["unit"] == "tokens/s" and j["higher_is_better"] is True and j["dtype"] == "bf16"
    # value and ms_per_step describe the same 3 timed steps of 4 x 64 tokens
    assert j["value"] == pytest.approx(4 * 64 / (j["ms_per_step"] * 1e-3), rel=1e-3)
    assert not any(k.startswith("batch") for k in j["extra"]), j["extra"]
    assert j["extra"]["no_comm"] is None and j["comm"]["ranks_identical"] is None


def test_full_adds_the_second_batch_point(runs):
    j, _ = runs[2]
    assert j["full"] is True
    b = j["extra"]["batch2"]
    assert b["ms_per_step"] > 0 and b["value"] > 0 and b["global_batch"] == 2


def test_dump_outputs_are_float32_arrays_of_the_last_step(runs):
    j, d = runs[0]
    arrs = {n: np.load(os.path.join(d, n + ".npy")) for n in NAMES}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
    assert arrs["loss"].shape == (1,) and arrs["grad_norm"].shape == (1,) and arrs["grad_norm"][0] > 0
    assert round(float(arrs["loss"][0]), 4) == j["loss"]
    index = json.load(open(os.path.join(d, "params_index.json")))
    assert sum(n for _, _, n, _ in index) == arrs["params"].size
    assert all(0 < n <= total for _, _, n, total in index)
    offs = [o for _, o, _, _ in index]
    assert offs == sorted(offs) and offs[0] == 0


def test_dump_outputs_repeat_exactly_and_precede_the_full_passes(runs):
    (_, a), (_, b), (_, full) = runs
    for n in NAMES:
        x = np.load(os.path.join(a, n + ".npy"))
        np.testing.assert_array_equal(x, np.load(os.path.join(b, n + ".npy")), err_msg=n)
        np.testing.assert_array_equal(x, np.load(os.path.join(full, n + ".npy")), err_msg=n)
