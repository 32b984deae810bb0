"""bench.py end to end on the GPU at a small batch: a plain run times exactly --steps steps and carries nothing that needs runs of its own, --full
adds the roofline block and the launch count, and --dump-outputs writes the last timed step's outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def bench(*args):
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--batch", "16"] + list(args), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{") and '"metric"' in ln][-1])


def test_plain_run_full_run_and_dumped_outputs(tmp_path):
    plain = bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "a"))
    assert plain["steps"] == 3 and plain["warmup"] == 1 and plain["ms_per_step"] > 0 and plain["value"] > 0
    assert plain["unit"] == "pairs/s" and plain["higher_is_better"] is True and plain["dtype"] == "bf16"
    assert abs(plain["value"] - 16 * 1e3 / plain["ms_per_step"]) <= 1e-3 * plain["value"]
    assert plain["roofline"] is None and plain["launches_per_step"] is None and plain["cpu_baseline"] is None and "parity_mode" not in plain
    names = ["img_f", "txt_f", "vis_prompt", "txt_prompt", "base_loss", "alignment_loss"] + [f"{kind}.{k}" for kind in ("grad", "param") for k in
                                                                                               ("dim_1_share", "dim_2_visual", "dim_2_textual", "dim_3_visual", "dim_3_textual")]
    assert sorted(os.listdir(tmp_path / "a")) == sorted(n + ".npy" for n in names)
    out = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in names}
    assert all(x.dtype == np.float32 and np.isfinite(x).all() for x in out.values())
    assert out["img_f"].shape == (16, 512) and out["txt_f"].shape == (16, 512) and out["base_loss"].shape == ()
    # the dump is the state after warmup + steps SGD updates: the same four steps split differently give the same outputs
    full = bench("--steps", "2", "--warmup", "2", "--full", "--no-cpu-baseline", "--no-extras", "--dump-outputs", str(tmp_path / "b"))
    for n in names:
        np.testing.assert_allclose(np.load(tmp_path / "b" / (n + ".npy")), out[n], rtol=1e-5, atol=1e-7, err_msg=n)
    assert full["steps"] == 2 and full["roofline"] is not None and full["roofline"]["achieved"] > 0 and full["launches_per_step"] > 0
    assert full["cpu_baseline"] is None and "parity_mode" not in full          # --no-cpu-baseline / --no-extras still thin a --full run out
