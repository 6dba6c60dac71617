"""bench.py on the device: a plain run times the --steps steps once and dumps what the timed path returned; --full
adds the roofline, the CPU baseline with parity, the PCIe-inclusive leg and the other precisions."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

BENCH = os.path.join(ROOT, "bench.py")
SMALL = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "2", "--height", "64", "--width", "96"]


def run(args, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    r = subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_dumps_the_masks_it_timed(tmp_path, syn, oracle):
    d = run(SMALL + ["--dump-outputs", str(tmp_path)])
    assert d["value"] > 0 and d["steps"] == 3 and len(d["ms_per_step_samples"]) == 1
    assert abs(d["value"] - 2 * 1e3 / d["ms_per_step"]) < 1e-6 * d["value"]
    assert d["roofline"] is None and d["cpu_baseline"] is None and "legs" not in d and "end_to_end" not in d
    mask = np.load(tmp_path / "mask.npy")
    assert mask.dtype == np.float32 and mask.shape == (2, 64, 96)
    # the same seeded frames and weights through the oracle
    sd = syn.make_state_dict(3, 3, True, 2)
    ref = oracle.torch_forward(sd, syn.frames_to_chw_f32(syn.make_frames_u8(2, 64, 96, "smooth", 1234, first=0)))
    ref_mask, _, _ = oracle.masks_from_logits(ref)
    bad = (mask != ref_mask) & (oracle.top2_margin(ref) > 2e-3)
    assert not bad.any()


def test_full_run_keeps_every_leg():
    d = run(SMALL + ["--full", "--cpu-frames", "2"])
    assert d["value"] > 0 and len(d["ms_per_step_samples"]) == 3
    assert d["roofline"]["launches"] > 0 and d["kernels"]
    assert d["cpu_baseline"]["value"] > 0 and d["parity"]["flips_outside_near_ties"] == 0
    assert d["end_to_end"]["mask_equals_resident_path"] is True
    assert set(d["legs"]) == {"exact8", "fast"} and all("value" in leg for leg in d["legs"].values())
