"""GPU: k_compact_hits (csrc/project.hip) under every span the launch can take, on a batch built around the places where a wave's
offset sums change shape: a frame without a hit, hits in a frame's last, partial wave-chunk, hits in the wave-chunks on both sides of
a seam between two groups of 16, and 32 masks in every frame (a full plane of mask bits).  The expectation is the CPU oracle's pass
over the same frames (tests/helpers.py)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

_SCRIPT = """
import sys
sys.path.insert(0, {root!r})
import numpy as np
from cm3d_amd import lifting, synthetic as syn
from oracle import oracle as orc
from tests.helpers import oracle_batch
WC, GRP = 256, 16                      # rows per wave-chunk, wave-chunks per group (csrc/project.hip)
cfg = syn.config("tiny", n_points=3050, n_masks=32, empty_mask_prob=0.0)
frames = [syn.make_frame(cfg, 40 + i) for i in range(4)]
bare = syn.make_frame(syn.config("tiny", n_points=3050, n_masks=32, empty_mask_prob=0.0, seed=99), 7)
bare.sweeps_raw = [np.ascontiguousarray(s * np.array([1, 1, 0, 1, 1], np.float32) + np.array([0, 0, 500, 0, 0], np.float32)) for s in bare.sweeps_raw]
frames.insert(2, bare)                 # every point 500 m up: in front of no camera's masks
lanes = [syn.make_lane_table(frames[0].ego_xyz[:2], 2000, seed=1)]
hb = lifting.pack_frames(frames, lanes, [0] * len(frames))
exp = oracle_batch(orc, frames, lanes, [0] * len(frames), hb)
n_masks = np.diff(hb.mask_off)
assert (n_masks == 32).all(), n_masks
seam = last = False
for fi, fr in enumerate(frames):
    rows = sum(s.shape[0] for s in fr.sweeps_raw)
    assert rows == 6100 and rows % WC and rows > GRP * WC
    dropped = rows - int(exp["pt_off"][fi + 1] - exp["pt_off"][fi])
    idx = np.concatenate([exp["hit_idx"][exp["hit_off"][m]:exp["hit_off"][m + 1]] for m in range(hb.mask_off[fi], hb.mask_off[fi + 1])] + [np.zeros(0, np.int32)])
    if fi == 2:
        assert idx.size == 0
        continue
    # a listed index i is row i .. i + dropped of the frame
    below = ((idx >= (GRP - 1) * WC) & (idx + dropped < GRP * WC)).any()
    above = ((idx >= GRP * WC) & (idx + dropped < (GRP + 1) * WC)).any()
    seam |= bool(below and above)
    last |= bool((idx >= (rows // WC) * WC).any())
assert seam and last, (seam, last)
if {gpu}:
    import torch
    from tests.test_gpu_parity import _compare
    eng = lifting.LiftEngine()
    eng.upload(hb)
    eng.run(masks="rle")
    torch.cuda.synchronize()
    eng.check_status()
    _compare(hb, eng.download(), exp)
print("SEAMS OK")
"""


@pytest.mark.parametrize("span", ["2", "4", "8"])
def test_compaction_at_its_seams_equals_the_oracle(span):
    """CM3D_CP_SPAN = 2 / 4 / 8 (read once per process, hence the child): index lists, coordinates and everything behind them equal the
    oracle's on the batch described at the top; the child also checks on the oracle's lists that the batch holds the cases it is for."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _SCRIPT.format(root=root, gpu=True)], env=dict(os.environ, CM3D_CP_SPAN=span), capture_output=True,
                       text=True, timeout=600, cwd=root)
    assert r.returncode == 0 and "SEAMS OK" in r.stdout, r.stderr[-3000:]
