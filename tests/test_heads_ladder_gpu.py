"""Every rung of the two layout ladders the multi-head HIP units share (csrc/heads_steps.h), once
per op that climbs it, on the MI355X:
  by_score_layout  sddmm_csr_heads and gatv2_scores_csr_heads: the nine fast rungs (leaves
                   1, 2, 4, ..., 256), the five general ones (leaves 1, 3, 5, 17, 65), and fast
                   shapes pushed onto the general path by a base one element off the alignment
  by_lane_group    spmm_csr_heads and gatv2_scores_csr_heads_grad (with and without p): lanes
                   1, 4, 16, 32, 64 and a second column tile, under the default schedule and under
                   split = chunk = 8, where hub chunks and the hub sum run
The checks are heads_cases' and gatv2_cases': bit for bit against the per-head loop, the reference
chain and the kCPU entries, on those modules' own row lengths."""
from __future__ import annotations

import pytest

import gatv2_cases as gc
import heads_cases as hc
from reduce_helpers import assert_same

pytestmark = pytest.mark.gpu

K = 256  # columns of the SDDMM's / SpMM's problem: above the longest row (130), small buffers

# (H, D, shift): leaves = H*D / 8 on the fast path
FAST = [(1, 8, 0), (2, 8, 0), (4, 8, 0), (8, 8, 0), (8, 16, 0), (8, 32, 0), (8, 64, 0), (16, 64, 0),
        (8, 256, 0)]
# leaves = ceil(D / 8) of one head; D / 8 is not a power of two
GENERAL = [(2, 5, 0), (2, 24, 0), (2, 40, 0), (2, 136, 0), (2, 520, 0)]
SHIFTED = [(8, 16, 1), (8, 64, 1), (8, 256, 1)]
SCORES = [(h, d, dt, "i32", shift) for (h, d, shift) in FAST + GENERAL + SHIFTED
          for dt in ("f32", "bf16")] + [(8, 16, "f32", "i64", 0)]

# lanes = H*D / (16 bytes of T): 1, 4, 16, 32, 64, 128 (two tiles)
LANES = [(h, d, "f32", "i32") for (h, d) in [(1, 4), (2, 8), (4, 16), (8, 16), (4, 64), (8, 64)]] + \
        [(h, d, "bf16", "i32") for (h, d) in [(1, 8), (4, 8), (8, 16), (8, 32), (8, 64), (16, 64)]] + \
        [(4, 16, "f32", "i64")]
SCHEDULES = ("default", "split8")


@pytest.mark.parametrize("h,d,dt,it,shift", SCORES)
def test_score_ladder_sddmm(device, h, d, dt, it, shift):
    hc.check_sddmm(device, h, d, dt, it, shift=shift, k=K)


@pytest.mark.parametrize("h,d,dt,it,shift", SCORES)
def test_score_ladder_gatv2_scores(device, h, d, dt, it, shift):
    if not shift:
        gc.check_forward(device, h, d, dt, it)
        return
    rp, ci, x_row, x_col, att, _ = p = gc.problem(h, d, dt, it)
    assert_same(gc.run_scores(device, *p[:5], 0.2, h, shift=1),
                gc.ref_scores(rp, ci, x_row, x_col, att, 0.2, h), f"scores H={h} D={d} {dt} shifted")


@pytest.mark.parametrize("h,d,dt,it", LANES)
def test_lane_ladder_spmm(device, h, d, dt, it):
    hc.check_spmm(device, h, d, dt, it, schedules=SCHEDULES, k=K)


@pytest.mark.parametrize("h,d,dt,it", LANES)
def test_lane_ladder_gatv2_grad(device, h, d, dt, it):
    gc.check_grad(device, h, d, dt, it, schedules=SCHEDULES, unaligned=False)
