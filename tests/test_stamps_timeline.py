"""tools/gemm_phase_stamps.py: the timeline arithmetic on synthetic stamps
(no GPU: the figures are plain differences of 100 MHz clock values)."""
import importlib.util
import os

import numpy as np

from tests.conftest import REPO_ROOT


def load_tool():
    spec = importlib.util.spec_from_file_location(
        "gemm_phase_stamps",
        os.path.join(REPO_ROOT, "tools", "gemm_phase_stamps.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def synthetic(tool):
    gemm = np.zeros(tool.SHAPE, dtype=np.int64)
    aux = np.zeros(tool.AUX_SHAPE, dtype=np.int64)
    t0 = 1_000_000
    # gate: two blocks, 0..10 us and 1..12 us
    aux[0, 0] = (t0, t0 + 1000)
    aux[0, 1] = (t0 + 100, t0 + 1200)
    # up: block 0 walks two jobs 14..40 and 40..70 us; block 9 has an empty
    # first job and runs only its second, 16..60 us
    gemm[0, 0, 0] = (t0 + 1400, t0 + 1500, t0 + 3800, t0 + 4000)
    gemm[0, 0, 1] = (t0 + 4000, t0 + 4400, t0 + 6700, t0 + 7000)
    gemm[0, 9, 1] = (t0 + 1600, t0 + 1700, t0 + 5800, t0 + 6000)
    # down: one block 75..120 us
    gemm[1, 3, 0] = (t0 + 7500, t0 + 7600, t0 + 11800, t0 + 12000)
    # combine: one block 123..128 us
    aux[1, 0] = (t0 + 12300, t0 + 12800)
    return gemm, aux


def test_forward_timeline_figures():
    tool = load_tool()
    tl = tool.forward_timeline(*synthetic(tool))
    assert tl["gate.first"] == 0.0 and tl["gate.span"] == 12.0
    assert tl["up.first"] == 14.0 and tl["up.last"] == 70.0
    assert tl["up.dead_before"] == 2.0      # gate's last exit 12 -> 14
    assert tl["down.dead_before"] == 5.0    # 70 -> 75
    assert tl["combine.dead_before"] == 3.0
    assert tl["total"] == 128.0
    # block walks 56 and 44 us; entry skew 0 and 2; idle tails 0 and 10
    assert tl["up.walk.max"] == 56.0 and tl["up.walk.p50"] == 50.0
    assert tl["up.skew.max"] == 2.0
    assert tl["up.tail.max"] == 10.0
    assert tl["up.walk.xcd0"] == 56.0 and tl["up.walk.xcd1"] == 44.0
    assert np.isnan(tl["up.walk.xcd2"])
    spans = sum(tl[k + ".span"] for k in ("gate", "up", "down", "combine"))
    deads = sum(tl[k + ".dead_before"] for k in ("up", "down", "combine"))
    assert spans + deads == tl["total"]


def test_forward_timeline_needs_all_four_kernels():
    tool = load_tool()
    gemm, aux = synthetic(tool)
    aux[1] = 0  # no combine record (e.g. the single-launch path ran)
    assert tool.forward_timeline(gemm, aux) is None
