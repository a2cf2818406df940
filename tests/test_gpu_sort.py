"""gscream_amd.scene_init.sort_keys (gsr_sort_keys_u64: stable LSD radix sort of unsigned 64-bit keys) bit-equal to torch.sort.

torch.sort has no uint64 kernel, so the yardstick sorts the int64 view with the top bit flipped (the order of the unsigned patterns)
and flips it back; every comparison is torch.equal on the int64 views.  B = SORT_BLOCK_KEYS is the workgroup's key count, imported."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gscream_amd import scene_init as SI  # noqa: E402
from gscream_amd.scene_init import SORT_BLOCK_KEYS as B  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOP = -(1 << 63)  # bit 63 as an int64


def torch_sorted(keys):
    """torch.sort in the order of the unsigned 64-bit patterns."""
    return torch.sort(keys ^ TOP).values ^ TOP


def random_keys(n, seed):
    g = torch.Generator().manual_seed(seed)
    lo = torch.randint(0, 1 << 32, (n,), generator=g, dtype=torch.int64)
    hi = torch.randint(0, 1 << 32, (n,), generator=g, dtype=torch.int64)
    return ((hi << 32) | lo).to(DEV)  # all 64 bits random: bit 63 is set in half of them


def check(keys):
    before = keys.clone()
    got = SI.sort_keys(keys)
    assert got.dtype == keys.dtype and got.shape == keys.shape
    assert torch.equal(keys, before)  # the input is left as it is
    assert torch.equal(got, torch_sorted(keys))
    return got


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, B - 1, B, B + 1, 3 * B + 17, 40 * B + 3])
def test_random_full_range_keys(n):
    """(40 B + 3: the 256 x workgroups counts no longer fit one tile of the count scan.)"""
    keys = random_keys(n, seed=n)
    if n > 64:
        assert 0.3 < float((keys < 0).float().mean()) < 0.7
    got = check(keys)
    again = SI.sort_keys(keys.view(torch.uint64))  # the same bits through the other dtype, and a second time
    assert again.dtype == torch.uint64 and torch.equal(again.view(torch.int64), got)


@pytest.mark.parametrize("bit", [0, 63])
def test_keys_that_differ_in_one_bit_only(bit):
    n = B + 77
    g = torch.Generator().manual_seed(bit)
    flip = torch.randint(0, 2, (n,), generator=g, dtype=torch.int64)
    keys = (torch.full((n,), 0x0123456789ABCDEF, dtype=torch.int64) ^ (flip * (TOP if bit == 63 else 1))).to(DEV)
    assert 0 < int(flip.sum()) < n
    check(keys)  # seven of the eight passes find their digit constant


def signed(x):
    """An unsigned 64-bit pattern as the int64 that holds it."""
    return x - (1 << 64) if x >> 63 else x


@pytest.mark.parametrize("digit", [0, 3, 7])
def test_a_constant_digit_is_a_skipped_pass(digit):
    field = 0xFF << (8 * digit)
    keys = (random_keys(2 * B + 5, seed=20 + digit) & signed(~field & ((1 << 64) - 1))) | signed(0xA5 << (8 * digit))
    check(keys)
    check(random_keys(2 * B + 5, seed=30 + digit) & signed(field))  # and the other way round: the one digit that varies


def test_duplicate_runs_cross_every_workgroup_boundary():
    n = 4 * B + 5
    g = torch.Generator().manual_seed(5)
    values = random_keys(7, seed=6).cpu()
    keys = values[torch.randint(0, 7, (n,), generator=g)].to(DEV)
    got = check(keys)
    assert int(torch.unique(got).numel()) == 7  # runs of ~B / 2 .. B keys: every workgroup boundary lies inside one


def test_sorted_and_reversed_input():
    keys = torch_sorted(random_keys(3 * B + 1, seed=8))
    check(keys)
    check(keys.flip(0).contiguous())
    assert torch.equal(SI.sort_keys(keys.flip(0).contiguous()), keys)


def test_all_keys_equal_skips_every_pass():
    keys = torch.full((B + 3,), -12345, dtype=torch.int64, device=DEV)
    check(keys)


def test_sixteen_million_keys():
    n = (1 << 24) + 5
    g = torch.Generator(device=DEV).manual_seed(11)
    draw = lambda: torch.randint(0, 1 << 32, (n,), generator=g, dtype=torch.int64, device=DEV)
    keys = (draw() << 32) | draw()
    assert torch.equal(SI.sort_keys(keys), torch_sorted(keys))


def test_sort_keys_never_stops_the_host():
    keys = random_keys(5 * B + 9, seed=13)
    SI.sort_keys(keys)  # library loading and first allocations out of the way
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a = SI.sort_keys(keys)
        b = SI.sort_keys(keys)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert torch.equal(a, b) and torch.equal(a, torch_sorted(keys))  # and the same call twice gives identical bits
