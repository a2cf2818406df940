"""CPU tests of the cross-attention anchor sampler (gscream_amd/anchor_sampler.py, torch path), of run_crossattn_rows and of the new
C symbols.

The yardstick for the semantics is the per-anchor loop of tests/anchor_sampler_helpers.py, written from the rules.  The reference's
block (train.py:436-511) is inline in training() and cannot be executed offline, so no reference-run vector exists."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import anchor_sampler_helpers as AH  # noqa: E402

NEW_SYMBOLS = ("gsr_anchor_sample_workspace_bytes", "gsr_anchor_sample")


def run_torch(scene, max_pairs, seed):
    from gscream_amd import anchor_sampler as AS
    visible, x, y, gt, rect = scene
    out = AS.sample_crossattn_anchors(*AH.to_torch(visible, x, y, gt), rect, max_pairs=max_pairs, seed=seed)
    assert AS.last_path == "torch"
    return out


def check_against_loop(out, scene, max_pairs, seed):
    """Everything the issue's 'Selection' list asks, against the loop.  -> the loop's result."""
    visible, x, y, gt, rect = scene
    ref = AH.sample_loop(visible, x, y, gt, rect, max_pairs, seed)
    src_mask, dst_mask, src_rows, dst_rows, info = out
    N = len(visible)
    assert src_mask.dtype == dst_mask.dtype == torch.bool and src_mask.shape == dst_mask.shape == (N,)
    assert src_rows.dtype == dst_rows.dtype == torch.int64 and src_rows.shape == dst_rows.shape == (max_pairs,)
    assert info.dtype == torch.int32 and info.tolist() == AH.info_list(ref), (info.tolist(), AH.info_list(ref))
    src, dst = torch.nonzero(src_mask.cpu()).reshape(-1).tolist(), torch.nonzero(dst_mask.cpu()).reshape(-1).tolist()
    n = ref["min_num"] if ref["ok"] else 0
    assert len(src) == len(dst) == n
    assert set(src) <= set(ref["fg"]) and set(dst) <= set(ref["bg"])
    assert src_rows[:n].tolist() == src and dst_rows[:n].tolist() == dst      # the rows are the ascending nonzeros of the masks
    assert src == ref["src"] and dst == ref["dst"]                            # the min_num smallest (key, index) of each class
    if ref["ok"] and ref["min_num"] == len(ref["fg"]):
        assert src == ref["fg"]
    if ref["ok"] and ref["min_num"] == len(ref["bg"]):
        assert dst == ref["bg"]
    return ref


def edge_scene():
    """Every rule of the classification on a 9 x 12 image: positions exactly 0, exactly w, w - 0.5, negative, NaN; invisible anchors
    with in-range positions; mask values 0, 1, 0.5, 2, -1; then enough ordinary anchors for both classes to pass 11."""
    h, w = 9, 12
    gt = np.zeros((h, w), dtype=np.float32)
    gt[:, 0:3], gt[:, 3:5], gt[:, 5:7], gt[:, 7:9] = 1.0, 0.5, 2.0, -1.0     # columns 9..11 stay 0
    pts = [  # (x, y, visible)
        (0.0, 4.0, True), (4.0, 0.0, True), (float(w), 4.0, True), (4.0, float(h), True), (w - 0.5, 4.5, True), (3.5, h - 0.5, True),
        (-1.0, 4.0, True), (4.0, -0.25, True), (float("nan"), 4.0, True), (4.0, float("nan"), True), (np.nextafter(np.float32(0), np.float32(1)), 4.0, True),
        (1.5, 4.5, False), (10.5, 2.5, False),
        (1.5, 1.5, True), (3.5, 1.5, True), (4.99, 2.5, True), (5.5, 3.5, True), (6.999, 3.5, True), (7.5, 3.5, True), (8.5, 8.5, True),
        (9.0, 1.0, True), (2.999, 7.0, True), (0.999, 0.999, True),
    ]
    rng = np.random.default_rng(5)
    for _ in range(60):
        pts.append((float(rng.uniform(0.01, w - 0.01)), float(rng.uniform(0.01, h - 0.01)), bool(rng.random() < 0.9)))
    x = np.array([p[0] for p in pts], dtype=np.float32)
    y = np.array([p[1] for p in pts], dtype=np.float32)
    visible = np.array([p[2] for p in pts])
    return visible, x, y, gt


@pytest.mark.parametrize("rect", [(0, 9, 0, 12), (-3, 40, 2, 50), (1, 8, 1, 11), (4, 4, 0, 12), (6, 2, 0, 12), (0, 9, 12, 30)])
def test_classes_and_counts_equal_the_loop_on_a_scene_that_hits_every_rule(rect):
    """Full image, a rectangle clipped by the image edge, an inner one, an empty one, an inverted one, one beside the image."""
    visible, x, y, gt = edge_scene()
    scene = (visible, x, y, gt, rect)
    ref = check_against_loop(run_torch(scene, 2000, seed=0x1234_5678_9ABC_DEF0), scene, 2000, 0x1234_5678_9ABC_DEF0)
    if rect == (0, 9, 0, 12):
        assert ref["ok"] and len(ref["fg"]) + len(ref["bg"]) < ref["n_sampled"]   # the -1 columns are sampled and in neither class
        assert 13 in ref["fg"] and 16 in ref["fg"] and 17 in ref["fg"]            # mask 1 and mask 2
        assert 14 in ref["bg"] and 4 in ref["bg"]                                 # mask 0.5 truncates to 0; x = w - 0.5 is the last column
        assert not {0, 1, 2, 3, 6, 7, 8, 9, 11, 12} & set(ref["fg"] + ref["bg"])  # on / outside the border, NaN, invisible
        assert 10 in ref["fg"] and 5 in ref["bg"]                                 # the smallest positive x; y = h - 0.5 is the last row
    if rect in ((4, 4, 0, 12), (6, 2, 0, 12), (0, 9, 12, 30)):
        assert ref["n_sampled"] == 0 and not ref["ok"]


@pytest.mark.parametrize("n_fg,n_bg,max_pairs", [(13, 300, 17), (40, 300, 17), (300, 40, 2000), (250, 250, 100), (64, 64, 64)])
def test_selection_is_the_smallest_keys_of_each_class(n_fg, n_bg, max_pairs):
    scene = AH.counted_scene(2000, n_fg, n_bg, seed=n_fg + n_bg)
    seed = 0xDEAD_BEEF_0000_0001 * (n_fg + 1) & (2 ** 64 - 1)
    ref = check_against_loop(run_torch(scene, max_pairs, seed), scene, max_pairs, seed)
    assert (len(ref["fg"]), len(ref["bg"])) == (n_fg, n_bg) and ref["min_num"] == min(n_fg, n_bg, max_pairs)


@pytest.mark.parametrize("n_fg,n_bg,ok", [(11, 40, False), (12, 40, True), (40, 11, False), (12, 12, True), (0, 0, False)])
def test_ok_needs_more_than_eleven_of_each_class(n_fg, n_bg, ok):
    scene = AH.counted_scene(500, n_fg, n_bg, seed=3)
    out = run_torch(scene, 2000, seed=7)
    ref = check_against_loop(out, scene, 2000, 7)
    assert ref["ok"] == ok and (len(ref["fg"]), len(ref["bg"])) == (n_fg, n_bg)
    assert int(out[4][3]) == min(n_fg, n_bg)                                      # min_num is reported either way
    if not ok:
        assert not out[0].any() and not out[1].any()


def test_random_scenes_equal_the_loop():
    for s, (N, h, w, max_pairs) in enumerate([(1, 5, 7, 2000), (63, 11, 13, 5), (3000, 40, 60, 200), (3000, 40, 60, 2000)]):
        scene = AH.random_scene(N, h, w, seed=s, mask_values=(0.0, 1.0, 0.5, 2.0, -1.0))
        check_against_loop(run_torch(scene, max_pairs, seed=s * 0x9E37_79B9_7F4A_7C15), scene, max_pairs, s * 0x9E37_79B9_7F4A_7C15)


def test_key_function_is_the_documented_one_and_a_bijection():
    from gscream_amd import anchor_sampler as AS
    idx = torch.arange(0, 70000, dtype=torch.int64)
    for seed in (0, 1, 0xFFFF_FFFF_FFFF_FFFF, 0x0123_4567_89AB_CDEF):
        k = AS.anchor_keys(idx, seed)
        assert int(k.min()) >= 0 and int(k.max()) < 2 ** 32 and torch.unique(k).numel() == idx.numel()
        for i in (0, 1, 2, 63, 64, 4099, 69999):
            assert int(k[i]) == AH.key(seed, i)
    assert AH.key(0, 0) == 0 and AH.key(0, 1) == AH.mix(AH.mix(1))
    # the words of the header comment, the module docstring and the C header agree
    line = "key(i) = mix(((mix((i ^ s_lo) + s_hi)) + s_lo) ^ s_hi)"
    for path in ("gscream_amd/csrc/anchor_sample.hip", "gscream_amd/anchor_sampler.py", "include/gsraster.h"):
        text = open(os.path.join(ROOT, path)).read()
        assert line in text and "0x7feb352d" in text and "0x846ca68b" in text, path


def test_selection_is_uniform_over_the_class():
    """One class of 64 members scattered among 10^5 indices, 16 chosen, 512 seeds drawn after torch.manual_seed(0): every member's
    selection count lies in [69, 187] = 128 +- 6 sigma of Binomial(512, 1/4) (sigma = 9.8)."""
    from gscream_amd import anchor_sampler as AS
    N, h, w = 100_000, 4, 6
    rng = np.random.default_rng(11)
    members = np.sort(rng.choice(N, 64, replace=False))
    others = np.sort(rng.choice(np.setdiff1d(np.arange(N), members), 64, replace=False))
    gt = np.zeros((h, w), dtype=np.float32)
    gt[:, :3] = 1.0
    x = np.full(N, -1.0, dtype=np.float32)
    y = np.full(N, 1.5, dtype=np.float32)
    x[members], x[others] = 1.5, 4.5
    visible = np.ones(N, dtype=bool)
    args = AH.to_torch(visible, x, y, gt)
    torch.manual_seed(0)
    counts = torch.zeros(N, dtype=torch.int64)
    counts_bg = torch.zeros(N, dtype=torch.int64)
    for _ in range(512):
        src_mask, dst_mask, _sr, _dr, info = AS.sample_crossattn_anchors(*args, (0, h, 0, w), max_pairs=16)
        assert info.tolist()[:5] == [128, 64, 64, 16, 1]
        counts += src_mask
        counts_bg += dst_mask
    for c, who in ((counts, members), (counts_bg, others)):
        assert int(c.sum()) == 512 * 16 and int(c[torch.from_numpy(who)].sum()) == 512 * 16
        got = c[torch.from_numpy(who)]
        print("selection counts: min", int(got.min()), "max", int(got.max()))
        assert 69 <= int(got.min()) and int(got.max()) <= 187


def test_manual_seed_makes_the_draw_repeatable():
    from gscream_amd import anchor_sampler as AS
    scene = AH.counted_scene(3000, 200, 300, seed=2)
    args, rect = AH.to_torch(*scene[:4]), scene[4]
    torch.manual_seed(123)
    a = AS.sample_crossattn_anchors(*args, rect, max_pairs=50)
    a2 = AS.sample_crossattn_anchors(*args, rect, max_pairs=50)
    torch.manual_seed(123)
    b = AS.sample_crossattn_anchors(*args, rect, max_pairs=50)
    torch.manual_seed(124)
    c = AS.sample_crossattn_anchors(*args, rect, max_pairs=50)
    for t, u in zip(a, b):
        assert torch.equal(t, u)
    assert not torch.equal(a[0], a2[0]) and not torch.equal(a[0], c[0]) and not torch.equal(a[1], c[1])
    assert torch.equal(a[4], c[4])                                                # the counts do not depend on the seed
    d = AS.sample_crossattn_anchors(*args, rect, max_pairs=50, seed=99)
    e = AS.sample_crossattn_anchors(*args, rect, max_pairs=50, seed=99)
    assert torch.equal(d[0], e[0]) and torch.equal(d[3], e[3])
    # a [1, h, w] mask (the reference's gt_mask) is taken as its plane
    f = AS.sample_crossattn_anchors(args[0], args[1], args[2], args[3][None], rect, max_pairs=50, seed=99)
    assert torch.equal(d[0], f[0]) and torch.equal(d[1], f[1])


# ---- run_crossattn_rows against run_crossattn ------------------------------------------------------------------------------
def standin(N=40, seed=0):
    """The stand-in model the crossattn tests use (tests/test_crossattn.py standin)."""
    from bidirectional_cross_attention import BidirectionalCrossAttention
    from gscream_amd import standin_model as SM
    feat = torch.randn(N, 32, generator=torch.Generator().manual_seed(seed))
    m = SM.Model(N, K=2, dtype=torch.float32)
    with torch.no_grad():
        m._anchor_feat.copy_(feat)
    torch.manual_seed(5)
    m.crossattn = BidirectionalCrossAttention(dim=32, heads=8, dim_head=64, context_dim=32)
    fg, bg = torch.zeros(N, dtype=torch.bool), torch.zeros(N, dtype=torch.bool)
    fg[[1, 4, 5, 9, 20, 33]] = True
    bg[[0, 2, 7, 8, 21, 22, 23, 39]] = True
    return m, fg, bg


@pytest.mark.parametrize("is_ref", [True, False])
@pytest.mark.parametrize("ema", [0.03, 1.0])
def test_run_crossattn_rows_is_bit_identical_to_the_mask_form(is_ref, ema):
    from gscream_amd import crossattn as CA
    w = torch.randn(40, 32, generator=torch.Generator().manual_seed(9))
    results = []
    for rows in (False, True):
        m, fg, bg = standin()
        if rows:
            assert CA.run_crossattn_rows(m, torch.nonzero(fg).reshape(-1), torch.nonzero(bg).reshape(-1), ema=ema, is_ref=is_ref) is None
        else:
            CA.run_crossattn(m, fg, bg, ema=ema, is_ref=is_ref)
        assert m.crossattn.last_path == "torch"
        new = m._anchor_feat
        assert new.requires_grad and new.retains_grad
        (new * w).sum().backward()
        results.append((new.detach().clone(), new.grad.clone(), {k: p.grad for k, p in m.crossattn.named_parameters()}))
    (feat_a, grad_a, pa), (feat_b, grad_b, pb) = results
    assert torch.equal(feat_a, feat_b) and torch.equal(grad_a, grad_b)
    assert len(pa) == len(pb) == 8
    for k in pa:
        assert (pa[k] is None) == (pb[k] is None), k
        if pa[k] is not None:
            assert torch.equal(pa[k], pb[k]), k
    assert sum(p is not None and float(p.abs().max()) > 0 for p in pb.values()) == (8 if is_ref else 5)


def test_run_crossattn_rows_refuses_pe_and_issues_no_nonzero():
    from gscream_amd import crossattn as CA
    import inspect
    m, fg, bg = standin()
    with pytest.raises(NotImplementedError):
        CA.run_crossattn_rows(m, torch.nonzero(fg).reshape(-1), torch.nonzero(bg).reshape(-1), pe=True)
    src = inspect.getsource(CA.run_crossattn_rows)
    assert "index_select" in src and "index_copy_" in src and "nonzero(" not in src.split('"""')[2]


def test_crossattn_step_on_cpu():
    """The whole step on the torch paths: True and the rows' features rewritten, False and the model untouched when not ok."""
    from gscream_amd import anchor_sampler as AS
    from gscream_amd import crossattn as CA
    scene = AH.counted_scene(40, 14, 15, seed=4)
    args, rect = AH.to_torch(*scene[:4]), scene[4]
    m, _fg, _bg = standin()
    m2, _fg, _bg = standin()
    old = m._anchor_feat.detach().clone()
    torch.manual_seed(8)
    assert AS.crossattn_step(m, *args, rect, ema=0.03, is_ref=True, max_pairs=13) is True
    torch.manual_seed(8)
    src_mask, dst_mask, _sr, _dr, info = AS.sample_crossattn_anchors(*args, rect, max_pairs=13)
    assert info.tolist()[1:5] == [14, 15, 13, 1]
    CA.run_crossattn(m2, src_mask, dst_mask, ema=0.03, is_ref=True)
    assert torch.equal(m._anchor_feat.detach(), m2._anchor_feat.detach())
    touched = src_mask | dst_mask
    assert torch.equal(m._anchor_feat.detach()[~touched], old[~touched]) and not torch.equal(m._anchor_feat.detach()[touched], old[touched])
    scene = AH.counted_scene(40, 11, 15, seed=4)
    m, _fg, _bg = standin()
    leaf = m._anchor_feat
    assert AS.crossattn_step(m, *AH.to_torch(*scene[:4]), scene[4], ema=0.03, is_ref=True) is False
    assert m._anchor_feat is leaf and torch.equal(leaf.detach(), old)


def test_new_symbols_in_header_binding_and_library(native_lib):
    from gscream_amd import _abi, _native
    for s in NEW_SYMBOLS:
        assert s in _abi.header().functions, s
        assert s in _native.EXPORTED_SYMBOLS, s
        assert hasattr(native_lib, s), s
    assert native_lib.gsr_abi_version() == 9
    assert native_lib.gsr_anchor_sample_workspace_bytes(500_000, 2000) >= 2 * 500_000
    assert native_lib.gsr_anchor_sample_workspace_bytes(0, 2000) > 0 and native_lib.gsr_anchor_sample_workspace_bytes(-1, 2000) == 0
    # argument checks run before anything touches a device
    call = lambda N, H, W, max_pairs: native_lib.gsr_anchor_sample(N, H, W, None, None, None, None, 0, 1, 0, 1, max_pairs, 0, *([None] * 7))  # noqa: E731
    assert call(-1, 4, 4, 5) == -1 and b"bad sizes" in native_lib.gsr_last_error()
    assert call(4, 0, 4, 5) == -1 and call(4, 4, 4, -1) == -1
    assert call(4, 4, 4, 5) == -1 and b"NULL" in native_lib.gsr_last_error()
    assert call(0, 4, 4, 5) == -1                                                # info is required even for N = 0
