"""CPU tests of tests/split_planes.py: the host model of the split trunk's planes agrees with torch's float8_e5m2 cast, and
the per-element checker accepts correctly made planes and rejects the defects a rewrite of the lo stores could make."""
import pytest
import torch

from tests.split_planes import (EL, LO, assert_planes_equal, check_split, e5m2_bytes, e5m2_rne, expect_split_exact,
                                split)


def _values(M=2125, N=320, seed=0):
    """fp32 values of a trunk-like output (a 256-row tile tail of 77 rows), as float64"""
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(M, N, generator=gen) * 3).double()


def test_e5m2_rne_matches_torch():
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(1 << 20, generator=gen, dtype=torch.float64) * torch.exp2(torch.randint(-26, 8, (1 << 20,), generator=gen).double())
    x = x.float().double()
    assert torch.equal(e5m2_rne(x), x.float().to(LO).double())
    # ties (three significant bits, the last one set), the subnormal range and its lower edge, signs, zero
    k = torch.arange(-16, 16, dtype=torch.float64)
    ties = torch.cat([(m + 0.125 * (2 * j + 1)) * torch.exp2(k) for m in (1.0,) for j in range(4)])
    edge = torch.tensor([2.0 ** -17, 1.5 * 2.0 ** -17, 2.0 ** -18, 3 * 2.0 ** -18, 2.0 ** -16, 1.5 * 2.0 ** -16, 0.0],
                        dtype=torch.float64)
    t = torch.cat([ties, edge, -ties, -edge])
    assert torch.equal(e5m2_rne(t), t.float().to(LO).double())
    assert e5m2_rne(torch.tensor([2.0 ** -17])).item() == 0.0                # tie to even: zero
    assert e5m2_rne(torch.tensor([1.25 * 2.0 ** -17])).item() == 2.0 ** -16  # NOT flushed
    assert torch.equal(e5m2_bytes(t.float().to(LO).double()), t.float().to(LO).view(torch.uint8))


def test_split_matches_torch_cast():
    v = _values().float()
    hi, lo = split(v)
    assert torch.equal(hi, v.to(EL))
    assert torch.equal(lo.view(torch.uint8), (v - v.to(EL).float()).to(LO).view(torch.uint8))


def test_expect_split_exact_round_trip():
    v = _values().float().double()
    hi, lo = expect_split_exact(v)
    hs, ls = split(v.float())
    assert torch.equal(hi, hs) and torch.equal(lo, ls.view(torch.uint8))
    assert_planes_equal(hs, ls, hi, lo)
    with pytest.raises(AssertionError, match="exact in fp32"):
        expect_split_exact(torch.tensor([1.0 + 2.0 ** -30], dtype=torch.float64))


def _planes():
    v = _values()
    hi, lo = expect_split_exact(v.float().double())
    return v.float().double(), hi, lo


def test_check_split_accepts_correct_planes():
    v, hi, lo = _planes()
    check_split(hi, lo, v)
    check_split(hi, lo.view(LO), v)
    # with a reference uncertainty: 2^-26 relative (an fp32 sum's bound), tight on nearly every element
    check_split(hi, lo, v + v.abs() * 2.0 ** -27, err64=v.abs() * 2.0 ** -26)


def _rejects(hi, lo, v, what, row=None, block=None):
    with pytest.raises(AssertionError, match=what) as e:
        check_split(hi, lo, v)
    msg = str(e.value)
    if row is not None:
        assert f"row {row}," in msg, msg
    if block is not None:
        assert f"32-column block {block}," in msg, msg
    return msg


def test_check_split_rejects_zero_lo():
    v, hi, lo = _planes()
    _rejects(hi, torch.zeros_like(lo), v, "lo plane")


@pytest.mark.parametrize("shift", [4, 8])
def test_check_split_rejects_shifted_lo(shift):
    v, hi, lo = _planes()
    _rejects(hi, torch.roll(lo, shift, dims=1), v, "lo plane")


def test_check_split_rejects_swapped_blocks():
    v, hi, lo = _planes()
    bad = lo.clone()
    bad[:, 64:96], bad[:, 96:128] = lo[:, 96:128], lo[:, 64:96]
    _rejects(hi, bad, v, "lo plane", row=0, block=2)


def test_check_split_rejects_m_tail():
    v, hi, lo = _planes()
    tail = (v.shape[0] // 256) * 256                 # the 77 rows past the last full 256-row tile
    bad = lo.clone()
    bad[tail:] = 0
    msg = _rejects(hi, bad, v, "lo plane")
    assert f"256-row tile {tail // 256})" in msg, msg


def test_check_split_rejects_sign_flip():
    v, hi, lo = _planes()
    _rejects(hi, lo ^ 0x80, v, "lo plane")


def test_check_split_rejects_wrong_hi():
    v, hi, lo = _planes()
    bad = hi.clone()
    bad[300, 17] = -bad[300, 17]
    _rejects(bad, lo, v, "hi plane", row=300, block=0)


def test_check_split_refuses_a_vacuous_reference():
    v, hi, lo = _planes()
    with pytest.raises(AssertionError, match="too large"):
        check_split(hi, torch.zeros_like(lo), v, err64=v.abs() * 2.0 ** -12)


def test_assert_planes_equal_reports_the_element():
    v, hi, lo = _planes()
    bad = lo.clone()
    bad[2100, 300] ^= 1
    with pytest.raises(AssertionError, match=r"lo plane differs at row 2100, column 300 \(32-column block 9, 256-row tile 8\)"):
        assert_planes_equal(hi, bad, hi, lo)
