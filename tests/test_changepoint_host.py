"""rpsmf_amd.changepoint.find_changepoint, the single change-point search on the host, against a brute-force O(n^2) evaluation of the
same cost: sum over channels of (k - 1) log ms(1 .. k-1) + (n - k + 1) log ms(k .. n), ms floored at the smallest normal double,
ties to the lowest k.  CPU only."""

import numpy as np
import pytest

from rpsmf_amd.changepoint import find_changepoint

TINY = np.finfo(np.float64).tiny


def brute(x, min_distance=1):
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    n = x.shape[1]
    best, best_k = np.inf, None
    for k in range(1 + min_distance, n - min_distance + 2):      # 1-based first sample of the second segment
        cost = 0.0
        for row in x:
            a, b = row[:k - 1], row[k - 1:]
            cost += len(a) * np.log(max(np.mean(a * a), TINY)) + len(b) * np.log(max(np.mean(b * b), TINY))
        if cost < best:
            best, best_k = cost, k
    return best_k


@pytest.mark.parametrize("channels", [1, 7])
@pytest.mark.parametrize("n", [2, 3, 200])
def test_against_the_brute_force_search(channels, n):
    rng = np.random.default_rng(100 * channels + n)
    for trial in range(4):
        x = rng.standard_normal((channels, n))
        cut = int(rng.integers(1, n))
        x[:, cut:] *= 3.0 + trial
        k = find_changepoint(x)
        assert isinstance(k, int) and 2 <= k <= n
        assert k == brute(x)
        if n == 200 and channels == 7:
            assert abs(k - (cut + 1)) <= 3
    if channels == 1:
        assert find_changepoint(x[0]) == brute(x[0])


def test_min_distance_and_the_batched_form():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((6, 3, 80))
    x[:, :, 50:] *= 4.0
    x[2] = rng.standard_normal((3, 80))
    x[2, :, 2:] *= 50.0                       # its one change is two samples in: out of reach of min_distance = 5
    ks = find_changepoint(x)
    assert ks.shape == (6,) and ks.dtype == np.int64
    assert list(ks) == [brute(xi) for xi in x]
    ks5 = find_changepoint(x, min_distance=5)
    assert list(ks5) == [brute(xi, 5) for xi in x]
    assert ks[2] == 3 and ks5[2] != 3 and 6 <= ks5.min() and ks5.max() <= 76


def test_a_constant_zero_segment_costs_a_finite_amount():
    x = np.zeros((2, 40))
    x[:, 25:] = np.random.default_rng(1).standard_normal((2, 15))
    assert find_changepoint(x) == brute(x) == 26
    z = np.zeros(10)                                      # every k costs n log(tiny) up to rounding: the same k as the brute force
    assert find_changepoint(z) == brute(z)


def test_ties_go_to_the_lowest_k():
    x = np.array([1.0, 1.0, 1.0, 1.0, 1.0, 1.0])          # ms = 1 everywhere: cost 0 at every k
    assert find_changepoint(x) == 2
    x = np.array([2.0, 1.0, 1.0, 2.0])                     # k = 2 and k = 4 mirror each other: log 4 + 3 log 2 both
    assert brute(x) == 2 and find_changepoint(x) == 2
    assert find_changepoint(np.stack([x, x[::-1]])) == 2


def test_refusals():
    with pytest.raises(ValueError, match="only 'rms'"):
        find_changepoint(np.ones(5), statistic="mean")
    with pytest.raises(ValueError, match="n >= 2"):
        find_changepoint(np.ones(1))
    with pytest.raises(ValueError, match="n >= 2"):
        find_changepoint(np.ones((2, 5)), min_distance=3)
    with pytest.raises(ValueError, match="min_distance"):
        find_changepoint(np.ones(5), min_distance=0)
    with pytest.raises(ValueError, match="finite"):
        find_changepoint(np.array([1.0, np.nan, 2.0]))
    with pytest.raises(ValueError, match="must be"):
        find_changepoint(np.ones((1, 2, 3, 4)))
