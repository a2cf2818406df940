"""CPU tests of the helpers the training-size GPU tests rely on (tests/helpers.py): the key alignment of two decodes'
compacted rows, and the host restatement of the kNN kernel's Morton buckets."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers as H  # noqa: E402


def _flipped():
    # N = 3 anchors x K = 3 offsets; the "kernel" keeps key 1 and drops key 4, both within rounding of zero
    mask_ref = torch.tensor([1, 0, 1, 1, 1, 0, 0, 1, 1], dtype=torch.bool)
    mask_got = torch.tensor([1, 1, 1, 1, 0, 0, 0, 1, 1], dtype=torch.bool)
    nop_ref = torch.tensor([0.5, -2e-7, 0.3, 0.7, 3e-6, -0.4, -0.9, 0.2, 0.6], dtype=torch.float64).view(-1, 1)
    return mask_got, mask_ref, nop_ref


def test_align_decode_rows_on_a_hand_made_flipped_mask():
    mask_got, mask_ref, nop_ref = _flipped()
    al = H.align_decode_rows(mask_got, mask_ref, nop_ref)
    assert al.keys_got.tolist() == [0, 1, 2, 3, 7, 8] and al.keys_ref.tolist() == [0, 2, 3, 4, 7, 8]
    assert al.rows_got.tolist() == [0, 2, 3, 4, 5] and al.rows_ref.tolist() == [0, 1, 2, 4, 5]
    assert al.ambiguous.tolist() == [False, True, False, False, True, False, False, False, False]
    # per-row outputs that depend on the key only line up on the shared keys
    vals = torch.arange(9, dtype=torch.float64) * 10 + 1
    out_got, out_ref = vals[al.keys_got], vals[al.keys_ref]
    assert torch.equal(out_got[al.rows_got], out_ref[al.rows_ref])
    assert torch.equal(out_got[al.rows_got], vals[[0, 2, 3, 7, 8]])
    # the upstream field is zero on the flipped keys: either side's gather gives the same <output, upstream>
    (f,) = H.upstream_fields(9, (1,), al.ambiguous, torch.Generator().manual_seed(0), mean=1.0)
    assert f[al.ambiguous].abs().sum() == 0 and f[~al.ambiguous].abs().min() > 0
    assert torch.allclose((out_got * f[al.keys_got, 0]).sum(), (out_ref * f[al.keys_ref, 0]).sum(), rtol=0, atol=1e-12)


def test_align_decode_rows_rejects_a_flip_away_from_zero():
    mask_got, mask_ref, nop_ref = _flipped()
    nop_ref[4] = 0.25  # the dropped key is no longer ambiguous
    with pytest.raises(AssertionError, match="mask differs away from zero"):
        H.align_decode_rows(mask_got, mask_ref, nop_ref)
    with pytest.raises(AssertionError):
        H.align_decode_rows(mask_got[:8], mask_ref, nop_ref)
    same = H.align_decode_rows(mask_ref, mask_ref, nop_ref)
    assert torch.equal(same.rows_got, same.rows_ref) and not same.ambiguous.any()


def test_morton_bucket_counts_corners_and_totals():
    pts = np.array([[0, 0, 0], [4, 2, 1], [4, 0, 0], [0, 2, 0], [0, 0, 1], [2.1, 1.1, 0.6]], np.float32)
    c = H.morton_bucket_counts(pts)
    assert c.shape == (4096,) and c.sum() == len(pts)
    # x is bit 0 of each 3-bit digit, y bit 1, z bit 2; the top cell of every axis sets its four top digits
    assert c[0] == 1 and c[4095] == 1 and c[0b001001001001] == 1 and c[0b010010010010] == 1 and c[0b100100100100] == 1
    # (2.1, 1.1, 0.6) of (4, 2, 1): 10-bit cells 537, 562, 613 -> top four bits 1000, 1000, 1001, interleaved z y x per digit
    assert c[0b111000000100] == 1
