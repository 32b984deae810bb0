"""tests/poison.py on CPU tensors: the fill touches exactly the complement of the live set, same_bits tells NaN payloads apart, the index
replacement stays in range, and the two-arm runner names a dependence on dead memory, a written preserved region and an empty poison set."""
import pytest
import torch

import poison as P


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_fill_touches_exactly_the_complement_of_the_live_set(dtype):
    g = torch.Generator().manual_seed(0)
    t = torch.randn(11, 6, generator=g).to(dtype)
    before = t.clone()
    live = torch.zeros(11, 6, dtype=torch.bool)
    live[2:7, :4] = True
    n = P.fill_nan(t, ~live)
    assert n == 11 * 6 - 5 * 4
    assert bool(torch.isnan(t[~live]).all()) and not bool(torch.isnan(t[live]).any())
    assert P.same_bits(t[live], before[live])
    # a row mask covers whole rows; None covers everything; a view is filled in place
    u = before.clone()
    rows = torch.tensor([r >= 9 for r in range(11)])
    assert P.fill_nan(u, rows) == 2 * 6
    assert bool(torch.isnan(u[9:]).all()) and P.same_bits(u[:9], before[:9])
    assert P.fill_nan(u[:, 4:]) == 11 * 2 and bool(torch.isnan(u[:, 4:]).all()) and P.same_bits(u[:9, :4], before[:9, :4])
    with pytest.raises(AssertionError):
        P.fill_nan(u, torch.ones(6, dtype=torch.bool))      # a mask of another shape is a mistake of the case, not "no rows"


def test_same_bits_tells_nan_payloads_apart():
    a = torch.tensor([1.0, float("nan"), -0.0])
    assert P.same_bits(a, a.clone())
    assert not bool((a == a).all())                              # what a float comparison would say
    b = a.clone()
    b.view(torch.int32)[1] ^= 1                                  # another NaN payload
    assert bool(torch.isnan(b[1])) and not P.same_bits(a, b)
    assert not P.same_bits(torch.tensor([0.0]), torch.tensor([-0.0]))
    for dtype in (torch.bfloat16, torch.float16):
        h = a.to(dtype)
        g = h.clone()
        assert P.same_bits(h, g)
        g.view(torch.int16)[1] ^= 1
        assert bool(torch.isnan(g[1])) and not P.same_bits(h, g)
    assert not P.same_bits(a, a.half())                          # another type
    assert P.same_bits(torch.tensor([3, 4]), torch.tensor([3, 4])) and not P.same_bits(torch.tensor([3, 4]), torch.tensor([3, 5]))


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_other_index_is_different_and_in_range(dtype):
    for n in (2, 3, 50):
        t = torch.arange(n, dtype=dtype).repeat(2)
        before = t.clone()
        mask = torch.ones(2 * n, dtype=torch.bool)
        mask[:n] = False
        assert P.other_index(t, mask, n) == n
        assert torch.equal(t[:n], before[:n])
        assert bool((t[n:] != before[n:]).all()) and bool(((t[n:] >= 0) & (t[n:] < n)).all())
    with pytest.raises(AssertionError):
        P.other_index(torch.tensor([5]), None, 5)                # the array already holds an index out of range


def _case(read_dead=False, write_kept=False, poison_nothing=False, wrong=False):
    def case(arm):
        x = torch.arange(12.0).reshape(4, 3) + 1
        live = torch.tensor([True, True, False, False])
        if not poison_nothing:
            arm.dead(x, ~live)
        out = torch.zeros(4, 3)
        arm.preserve("out", out, ~live)
        out[:2] = 2 * x[:2] + (0.0 * x[2:] if read_dead else 0.0) + (1.0 if wrong else 0.0)      # 0 x stale: invisible with finite data
        if write_kept:
            out[3] = 0.0
        arm.out("y", out, live, ref=2 * (torch.arange(12.0).reshape(4, 3) + 1).double(), tol=1e-6)
    return case


def test_two_arm_runner_verdicts():
    assert P.two_arms(_case(), "ok") == 6
    with pytest.raises(AssertionError, match="depends on dead memory"):
        P.two_arms(_case(read_dead=True), "reads")
    with pytest.raises(AssertionError, match="preserved region was written"):
        P.two_arms(_case(write_kept=True), "writes")
    with pytest.raises(AssertionError):
        P.two_arms(_case(poison_nothing=True), "empty")
    with pytest.raises(AssertionError):
        P.two_arms(_case(wrong=True), "reference")
