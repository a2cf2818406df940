"""The cross-attention anchor sampler on the device (gsr_anchor_sample) against the torch path of the same module, bit for bit, and
`crossattn_step` end to end.  The torch path's own yardstick is the per-anchor loop (tests/test_anchor_sampler.py, CPU).

The reference's block (train.py:436-511) is inline in training() and cannot be executed offline, so no reference-run vector exists."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import anchor_sampler_helpers as AH  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -7777


def both_paths(scene, max_pairs, seed):
    """-> (hip result, torch-path result on the CPU copy of the same inputs), compared bit for bit."""
    from gscream_amd import anchor_sampler as AS
    visible, x, y, gt, rect = scene
    hip = AS.sample_crossattn_anchors(*AH.to_torch(visible, x, y, gt, DEV), rect, max_pairs=max_pairs, seed=seed)
    assert AS.last_path == "hip"
    ref = AS.sample_crossattn_anchors(*AH.to_torch(visible, x, y, gt), rect, max_pairs=max_pairs, seed=seed)
    assert AS.last_path == "torch"
    assert hip[4].is_cuda and hip[4].dtype == torch.int32 and hip[4].tolist() == ref[4].tolist(), (hip[4].tolist(), ref[4].tolist())
    n = int(ref[4][3]) if int(ref[4][4]) else 0
    for k in (0, 1):
        assert hip[k].dtype == torch.bool and torch.equal(hip[k].cpu(), ref[k]), ("mask", k)
    for k in (2, 3):
        assert hip[k].dtype == torch.int64 and hip[k].shape == (max_pairs,)
        assert torch.equal(hip[k][:n].cpu(), ref[k][:n]), ("rows", k)
        assert torch.equal(hip[k][:n].cpu(), torch.nonzero(ref[k - 2]).reshape(-1))          # ascending = the order of feat[mask]
        assert bool((hip[k][n:] == -1).all())
    return hip, ref


CASES = {
    "N1": lambda: (AH.random_scene(1, 5, 7, seed=1, frac_visible=1.0), 2000),
    "N63": lambda: (AH.counted_scene(63, 20, 25, seed=2), 2000),
    "N4099": lambda: (AH.counted_scene(4099, 700, 900, seed=3), 300),                      # several workgroups, a ragged tail
    "N4099_random": lambda: (AH.random_scene(4099, 40, 60, seed=4, mask_values=(0.0, 1.0, 0.5, 2.0, -1.0)), 2000),
    "N200003": lambda: (AH.random_scene(200_003, 64, 96, seed=5, mask_values=(0.0, 1.0, -1.0)), 2000),  # 782 blocks: one total per top-scan thread
    # 262 147 anchors = 1025 blocks of 256: the smallest size at which a top-scan thread owns two totals and the last run is ragged
    "N262147": lambda: (AH.random_scene(262_147, 64, 96, seed=13, mask_values=(0.0, 1.0, -1.0)), 2000),
    "N200003_whole_classes": lambda: (AH.random_scene(200_003, 64, 96, seed=6, rect=(10, 30, 5, 50)), 100_000),
    "cap17_class13": lambda: (AH.counted_scene(2000, 13, 300, seed=7), 17),                # min_num set by a class
    "cap17_class40": lambda: (AH.counted_scene(2000, 40, 300, seed=8), 17),                # min_num set by the cap
    "cap2000": lambda: (AH.counted_scene(8000, 2500, 3000, seed=9), 2000),                 # the reference's cap
    "not_ok": lambda: (AH.counted_scene(2000, 11, 300, seed=10), 2000),
    "empty_rect": lambda: (AH.random_scene(4099, 40, 60, seed=11, rect=(20, 20, 0, 60)), 2000),
}


@pytest.mark.parametrize("case", list(CASES))
def test_hip_equals_the_torch_path_bit_for_bit(case):
    scene, max_pairs = CASES[case]()
    seed = 0x9E37_79B9_7F4A_7C15 * (len(case) + 3) & (2 ** 64 - 1)
    hip, ref = both_paths(scene, max_pairs, seed)
    info = ref[4].tolist()
    print(case, "info", info)
    if case == "cap17_class13":
        assert info[1:5] == [13, 300, 13, 1]
    if case == "cap17_class40":
        assert info[1:5] == [40, 300, 17, 1]
    if case == "cap2000":
        assert info[1:5] == [2500, 3000, 2000, 1]
    if case == "not_ok":
        assert info[1:5] == [11, 300, 11, 0] and not hip[0].any() and not hip[1].any()
    if case in ("N200003", "N262147"):
        assert info[4] == 1 and info[3] == 2000 and min(info[1], info[2]) > 5000
    if case == "N200003_whole_classes":
        assert info[4] == 1 and info[3] == min(info[1], info[2]) > 2048                   # one side is its whole class
    if case == "empty_rect":
        assert info == [0] * 8


def test_no_anchors():
    from gscream_amd import anchor_sampler as AS
    gt = torch.ones(4, 6, device=DEV)
    e = torch.zeros(0, device=DEV)
    src_mask, dst_mask, src_rows, dst_rows, info = AS.sample_crossattn_anchors(e.bool(), e, e, gt, (0, 4, 0, 6), max_pairs=5, seed=1)
    assert AS.last_path == "hip" and src_mask.shape == dst_mask.shape == (0,) and info.tolist() == [0] * 8
    assert src_rows.tolist() == dst_rows.tolist() == [-1] * 5


def test_two_calls_with_one_seed_are_bit_identical_and_rows_ascend():
    from gscream_amd import anchor_sampler as AS
    visible, x, y, gt, rect = AH.random_scene(200_003, 64, 96, seed=12)
    args = AH.to_torch(visible, x, y, gt, DEV)
    a = AS.sample_crossattn_anchors(*args, rect, seed=42)
    b = AS.sample_crossattn_anchors(*args, rect, seed=42)
    c = AS.sample_crossattn_anchors(*args, rect, seed=43)
    for t, u in zip(a, b):
        assert torch.equal(t, u)
    n = a[4].tolist()[3]
    assert n == 2000 and bool((a[2][1:n] > a[2][:n - 1]).all()) and bool((a[3][1:n] > a[3][:n - 1]).all())
    assert not torch.equal(a[0], c[0]) and not torch.equal(a[1], c[1]) and torch.equal(a[4], c[4])
    torch.manual_seed(77)                       # seed=None draws from torch's CPU generator
    d = AS.sample_crossattn_anchors(*args, rect)
    torch.manual_seed(77)
    e = AS.sample_crossattn_anchors(*args, rect)
    assert torch.equal(d[0], e[0]) and torch.equal(d[3], e[3]) and not torch.equal(d[0], a[0])


def test_row_entries_from_min_num_on_are_left_untouched():
    from gscream_amd import anchor_sampler as AS
    for n_fg, n_bg, max_pairs, want in ((13, 300, 17, 13), (40, 300, 17, 17), (11, 300, 17, 0)):
        visible, x, y, gt, rect = AH.counted_scene(2000, n_fg, n_bg, seed=13)
        src_rows = torch.full((max_pairs,), SENTINEL, dtype=torch.int64, device=DEV)
        dst_rows = torch.full((max_pairs,), SENTINEL, dtype=torch.int64, device=DEV)
        out = AS._sample_hip(*AH.to_torch(visible, x, y, gt, DEV), rect, max_pairs, 5, src_rows, dst_rows)
        assert out[2] is src_rows and out[3] is dst_rows
        assert int(out[0].sum()) == int(out[1].sum()) == want
        for rows in (src_rows, dst_rows):
            assert bool((rows[want:] == SENTINEL).all()) and bool((rows[:want] >= 0).all())


def standin(N, seed=0):
    from bidirectional_cross_attention import BidirectionalCrossAttention
    from gscream_amd import standin_model as SM
    m = SM.Model(N, K=2, dtype=torch.float32, seed=seed)
    torch.manual_seed(5)
    m.crossattn = BidirectionalCrossAttention(dim=32, heads=8, dim_head=64, context_dim=32)
    return m.to(DEV)


def test_no_host_stop_inside_the_sampler_or_run_crossattn_rows():
    """torch.cuda.set_sync_debug_mode("error") makes every synchronising torch call raise: the HIP sampler and run_crossattn_rows
    run under it (after one untimed call of each, so that library loading and first allocations are out of the way)."""
    from gscream_amd import anchor_sampler as AS
    from gscream_amd import crossattn as CA
    visible, x, y, gt, rect = AH.counted_scene(4099, 700, 900, seed=14)
    args = AH.to_torch(visible, x, y, gt, DEV)
    m = standin(4099)
    out = AS.sample_crossattn_anchors(*args, rect, max_pairs=300, seed=3)
    n = out[4].tolist()[3]
    assert n == 300
    CA.run_crossattn_rows(m, out[2][:n], out[3][:n], ema=0.03, is_ref=True)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out2 = AS.sample_crossattn_anchors(*args, rect, max_pairs=300, seed=3)
        assert AS.last_path == "hip"
        CA.run_crossattn_rows(m, out2[2][:n], out2[3][:n], ema=0.03, is_ref=True)
        assert m.crossattn.last_path == "hip"
        with pytest.raises(RuntimeError):          # the mode is live: a read-back does raise
            out2[4].tolist()
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert torch.equal(out[0], out2[0]) and torch.equal(out[2], out2[2])


@pytest.mark.parametrize("is_ref", [True, False])
def test_crossattn_step_end_to_end(is_ref):
    from gscream_amd import anchor_sampler as AS
    from gscream_amd import crossattn as CA
    visible, x, y, gt, rect = AH.counted_scene(4099, 700, 900, seed=15)
    args = AH.to_torch(visible, x, y, gt, DEV)
    base = standin(4099)
    old = base._anchor_feat.detach().clone()
    m, m2 = copy.deepcopy(base), copy.deepcopy(base)
    torch.manual_seed(21)
    assert AS.crossattn_step(m, *args, rect, ema=0.03, is_ref=is_ref, max_pairs=300) is True
    assert AS.last_path == "hip" and m.crossattn.last_path == "hip"
    torch.manual_seed(21)
    src_mask, dst_mask, src_rows, dst_rows, info = AS.sample_crossattn_anchors(*args, rect, max_pairs=300)
    assert info.tolist()[1:5] == [700, 900, 300, 1]
    new = m._anchor_feat.detach()
    changed = (new != old).any(dim=1)
    want = (src_mask | dst_mask) if is_ref else dst_mask
    assert torch.equal(changed, want)                                   # only the selected rows; only bg rows when not is_ref
    CA.run_crossattn(m2, src_mask, dst_mask, ema=0.03, is_ref=is_ref)   # the mask form on the returned masks: the same bits
    assert m2.crossattn.last_path == "hip" and torch.equal(new, m2._anchor_feat.detach())
    assert m._anchor_feat.requires_grad and m._anchor_feat.retains_grad
    w = torch.randn(new.shape, generator=torch.Generator().manual_seed(9)).to(DEV)
    (m._anchor_feat * w).sum().backward()
    (m2._anchor_feat * w).sum().backward()
    for (k, p), (_k2, p2) in zip(m.crossattn.named_parameters(), m2.crossattn.named_parameters()):
        assert (p.grad is None) == (p2.grad is None), k
        if p.grad is not None:
            assert torch.equal(p.grad, p2.grad), k


def test_crossattn_step_returns_false_and_leaves_the_model_untouched_when_not_ok():
    from gscream_amd import anchor_sampler as AS
    visible, x, y, gt, rect = AH.counted_scene(4099, 700, 11, seed=16)
    m = standin(4099)
    leaf, old = m._anchor_feat, m._anchor_feat.detach().clone()
    m.crossattn.last_path = None
    assert AS.crossattn_step(m, *AH.to_torch(visible, x, y, gt, DEV), rect, ema=0.03, is_ref=True) is False
    assert AS.last_path == "hip" and m.crossattn.last_path is None
    assert m._anchor_feat is leaf and torch.equal(leaf.detach(), old)
