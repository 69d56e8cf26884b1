"""pcr_order_statistic on the GPU: the exact k-th smallest float64 key and the count of keys <= it, against np.sort.

Sizes: 1, 2, around one wave (63, 64, 65), around one block of 256 lanes (255, 256, 257), several blocks (1025, 4097), and one size
past the histogram grid's first stride.  The rule of that grid (select.h): ceil(n / 256) blocks of 256 lanes, at most 1024 -- so a
lane's second key lies 1024 * 256 = 262144 keys behind its first, whatever the device; 262144 + 257 keys give every lane of the
first block, and one lane of the second, a second trip.  Ranks: 1, 2, n / 2, n - 1, n (those that exist).

Expected, for every case: value == np.sort(keys)[k - 1] under == (so -0.0 for 0.0 passes, and nothing else does: == on float64 is
exact), and n_le == np.sum(keys <= value)."""

import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STRIDE = 1024 * 256
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1025, 4097, STRIDE + 257)


@pytest.fixture(scope="module")
def capi():
    from point_cloud_registration_amd import _capi
    assert _capi.device_count() >= 1, "no MI355X visible"
    return _capi


@pytest.fixture(scope="module")
def ctx(capi):
    return capi.get_context(0)


def ranks(m):
    return sorted({k for k in (1, 2, m // 2, m - 1, m) if 1 <= k <= m})


def check(capi, ctx, keys, what):
    """Every rank of the rule over the keys < inf; -> the results."""
    keys = np.ascontiguousarray(keys, dtype=np.float64)
    inside = keys[keys < np.inf]                       # (drops NaN too)
    ordered = np.sort(inside)
    got = []
    for k in ranks(len(inside)):
        value, n_le = capi.order_statistic(ctx, keys, k)
        want = ordered[k - 1]
        with np.errstate(invalid="ignore"):
            count = int(np.sum(keys <= want))
        assert value == want, (what, len(keys), k, value, want)
        assert n_le == count, (what, len(keys), k, n_le, count)
        got.append((value, n_le))
    return got


def key_sets(n, rng):
    """name -> n keys."""
    half = np.arange(n) % 2 == 1
    sets = {
        # 10^-300 .. 10^300: every exponent digit takes part
        "lognormal": 10.0 ** rng.uniform(-300.0, 300.0, n),
        "equal": np.full(n, 0.3125),
        # neighbours: the first seven digits agree, the last one decides
        "last_bit": np.where(half, np.nextafter(1.75, 2.0), 1.75),
        # ... and the other end: the top digit decides, the rest agree (2^-1000, 2^-500, 1, 2^500: sign + 7 exponent bits differ)
        "top_digit": np.array([2.0 ** -1000, 2.0 ** -500, 1.0, 2.0 ** 500])[rng.integers(0, 4, n)],
        "zeros_denormals": np.array([0.0, 5e-324, 1e-310, 2.2250738585072014e-308, 0.0])[rng.integers(0, 5, n)],
        "negative": np.concatenate([-(10.0 ** rng.uniform(-300.0, 300.0, n - n // 2)), np.array([-0.0, 0.0, 1e-300, -np.inf, 5e-324])[rng.integers(0, 5, n // 2)]]),
        "half_inf": np.where(half, np.inf, rng.lognormal(0.0, 4.0, n)),
        "nans": np.where(rng.random(n) < 0.3, np.nan, rng.normal(0.0, 1e5, n)),
    }
    return sets


@pytest.mark.parametrize("n", SIZES)
def test_order_statistic(capi, ctx, n):
    rng = np.random.default_rng(n)
    for name, keys in key_sets(n, rng).items():
        assert len(keys) == n
        if not np.any(keys < np.inf):
            continue                                   # (n = 1 with its one key inf or NaN: test_refusals)
        first = check(capi, ctx, rng.permutation(keys), name)
        if n in (257, 4097):
            assert check(capi, ctx, keys, name) == first           # (the order of the keys does not matter)


def test_every_key_distinct(capi, ctx):
    """4097 distinct keys, EVERY rank: the k-th smallest is ordered[k - 1] and exactly k keys are <= it."""
    rng = np.random.default_rng(1)
    keys = rng.permutation(np.concatenate([-(10.0 ** rng.uniform(-30, 30, 2000)), 10.0 ** rng.uniform(-30, 30, 2097)]))
    ordered = np.sort(keys)
    assert len(np.unique(keys)) == 4097
    for k in range(1, 4098, 37):
        assert capi.order_statistic(ctx, keys, k) == (ordered[k - 1], k)


def test_signed_zero_and_determinism(capi, ctx):
    keys = np.array([-0.0, 0.0, -1.0, 0.0, 2.0, -0.0])
    for k, (want, count) in zip(range(1, 7), [(-1.0, 1)] + [(0.0, 5)] * 4 + [(2.0, 6)]):
        value, n_le = capi.order_statistic(ctx, keys, k)
        assert value == want and n_le == count
    rng = np.random.default_rng(2)
    keys = rng.lognormal(0.0, 50.0, STRIDE + 257)
    a = capi.order_statistic(ctx, keys, 100000)
    b = capi.order_statistic(ctx, keys, 100000)
    assert np.float64(a[0]).tobytes() == np.float64(b[0]).tobytes() and a[1] == b[1]


def test_refusals(capi, ctx):
    """NULL arguments, n < 1, k < 1, k above the number of keys < +inf: PCR_ERR_INVALID and both outputs untouched."""
    L = capi.lib()
    keys = np.array([3.0, np.inf, 1.0, np.nan, 2.0])
    p = keys.ctypes.data_as(ctypes.c_void_p)

    def refused(ctx_h, keys_p, n, k, null_value=False, null_count=False):
        value, n_le = ctypes.c_double(7.25), ctypes.c_int64(-3)
        st = L.pcr_order_statistic(ctx_h, keys_p, n, k, None if null_value else ctypes.byref(value), None if null_count else ctypes.byref(n_le))
        assert st == capi.PCR_ERR_INVALID and value.value == 7.25 and n_le.value == -3, (n, k, st)

    refused(None, p, 5, 1)
    refused(ctx.handle, None, 5, 1)
    refused(ctx.handle, p, 5, 1, null_value=True)
    refused(ctx.handle, p, 5, 1, null_count=True)
    refused(ctx.handle, p, 0, 1)
    refused(ctx.handle, p, -1, 1)
    refused(ctx.handle, p, 5, 0)
    refused(ctx.handle, p, 5, -2)
    refused(ctx.handle, p, 5, 4)                       # three keys < inf
    refused(ctx.handle, p, 2, 2)                       # one of the first two
    with pytest.raises(ValueError):
        capi.order_statistic(ctx, keys, 4)
    with pytest.raises(ValueError):
        capi.order_statistic(ctx, np.array([np.inf, np.nan]), 1)
    assert capi.order_statistic(ctx, keys, 3) == (3.0, 3)
