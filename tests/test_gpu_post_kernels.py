"""The adaptive retirement check (k_retire_flag / _scan / _scatter) and the noise reduction (k_noise_stats, _counts, _final)
on synthetic moments, through rtx_device_retire / rtx_device_noise_reduce (the handle's own launch helpers), against numpy:
the compaction exactly, the reduction's sum bit for bit in its documented order (_noise_tree), at sizes from one pixel to
a 4K frame -- past 256 blocks, where k_retire_scan gives each thread several blocks and k_noise_stats_final several
partials."""
import numpy as np
import pytest

from test_gpu_progressive import _noise_tree, _rel_err

pytestmark = pytest.mark.gpu

SPP = 4
TARGET = 0.5
# nb = 1 .. 4 blocks, 256 (per = 1), 257 (per = 2: threads 129..255 own no block), 3907 (the README's 1000 x 1000), the 4K
# frame's 32400 (per = 127)
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025, 65535, 65536, 65537, 131073, 1000000, 8294400]
PATTERNS = ["none", "all", "alternating", "lane0", "lane63", "first", "last", "blocks", "one_wave", "p0.01", "p0.5", "p0.99"]
BIG = 1000000  # from here on a subset of the patterns (host memory and time)
BIG_PATTERNS = ["none", "lane63", "blocks", "one_wave", "p0.5"]


def _pattern(name, n, rng):
    k = np.arange(n)
    if name == "none":
        return np.zeros(n, dtype=bool)
    if name == "all":
        return np.ones(n, dtype=bool)
    if name == "alternating":
        return k % 2 == 0
    if name == "lane0":
        return k % 64 == 0
    if name == "lane63":
        return k % 64 == 63
    if name == "first":
        return k == 0
    if name == "last":
        return k == n - 1
    if name == "blocks":  # full blocks alternating with empty ones
        return (k // 256) % 2 == 0
    if name == "one_wave":  # one live wave per block, a different one in each block
        return (k // 64) % 4 == (k // 256) % 4
    return rng.random(n) < float(name[1:])


def _keep_moments(keep):
    """S, Q (npix x 3) whose r at SPP samples is exactly 0 (four equal samples: S = 2, Q = 1) where keep is False and
    about 0.99 (S = 2, Q = 4) where it is True."""
    S = np.full((keep.size, 3), 2.0)
    Q = np.where(keep[:, None], 4.0, 1.0) * np.ones((1, 3))
    return S, Q


def _random_moments(npix, rng, n=SPP):
    """Moments whose r spans about twelve decades: mean 1e-4 .. 1e2, coefficient of variation 1e-6 .. 10."""
    m = 10.0 ** rng.uniform(-4, 2, (npix, 3))
    cv = 10.0 ** rng.uniform(-6, 1, (npix, 3))
    S = n * m
    Q = S * S / n + (n - 1) * (m * cv) ** 2
    return S, Q


def _rel_err_each(S, Q, n):
    """_rel_err with each pixel at its own count n (an array)."""
    r = np.zeros(S.shape[0])
    for v in np.unique(n):
        sel = n == v
        r[sel] = _rel_err(S[sel], Q[sel], int(v))
    return r


def _retire(rtsr, S, Q, active, spp, target, counts0):
    """One check on the device against numpy: the survivors, in order; spp at the retired pixels, every other count
    unchanged.  -> (next, counts)."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        r = _rel_err(S[active], Q[active], spp)
    keep = ~(r <= target)
    nxt, counts = rtsr.device_retire(S, Q, active, spp, target, counts0)
    assert nxt.dtype == np.uint32 and nxt.size == int(keep.sum()), (nxt.size, int(keep.sum()))
    assert np.array_equal(nxt, active[keep])
    expect = np.array(counts0, dtype=np.int32)
    expect[active[~keep]] = spp
    assert np.array_equal(counts, expect), "%d counts differ" % int((counts != expect).sum())
    return nxt, counts


def _reduce(rtsr, S, Q, spp, target, counts=None):
    n = np.where(counts == 0, spp, counts) if counts is not None else np.full(S.shape[0], spp)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        r = _rel_err_each(S, Q, n)
    got = rtsr.device_noise_reduce(S, Q, spp, target, counts)
    ref = _noise_tree(r, target)
    assert got[0] == ref.max, (got[0], ref.max)
    assert got[2] == ref.above, (got[2], ref.above)
    assert got[1] == ref.sum, (got[1], ref.sum, got[1] - ref.sum)
    return got, r


@pytest.mark.parametrize("n", SIZES)
def test_retire_keep_patterns(rtsr, n):
    rng = np.random.default_rng(n)
    for name in (BIG_PATTERNS if n >= BIG else PATTERNS):
        keep = _pattern(name, n, rng)
        S, Q = _keep_moments(keep)
        r = _rel_err(S, Q, SPP)
        assert np.array_equal(r > TARGET, keep) and ((r == 0.0) | (r > 0.9)).all()
        counts0 = rng.choice(np.array([0, 0, 2, 3, 7], dtype=np.int32), n)  # earlier counts, active pixels' 0 among them
        active = np.arange(n, dtype=np.uint32)
        nxt, counts = _retire(rtsr, S, Q, active, SPP, TARGET, counts0)
        assert nxt.size == int(keep.sum()), name


@pytest.mark.parametrize("n", [k for k in SIZES if k <= BIG])
def test_retire_sparse_lists(rtsr, n):
    """Lists that are not the identity: every 3rd pixel of a larger frame, ending at its last pixel; random ascending
    subsets, one of them ending at npix - 1.  Pixels off the list keep their counts even where their r is 0."""
    rng = np.random.default_rng(1000 + n)
    lists = [(np.arange(2, 3 * n + 2, 3, dtype=np.uint32), 3 * n + 2)]  # (active, npix): ends at npix - 1
    if n <= 131073:
        for m in (n + n // 2 + 1, 6 * n):
            lists.append((np.sort(rng.choice(m, n, replace=False)).astype(np.uint32), m + 7))
        last = lists[-1][0].copy()
        last[-1] = 6 * n - 1
        lists.append((last, 6 * n))
    for active, npix in lists:
        S, Q = _keep_moments(_pattern("p0.5", npix, rng))
        counts0 = rng.choice(np.array([0, 2, 3, 9], dtype=np.int32), npix)
        _retire(rtsr, S, Q, active, SPP, TARGET, counts0)


def test_retire_is_deterministic_and_chains(rtsr):
    """The same case twice gives the same bytes; rounds at rising spp and targets, each on the list the last one left,
    follow a numpy walk of the rule."""
    rng = np.random.default_rng(7)
    for npix in (65537, 1000000):
        S, Q = _random_moments(npix, rng, n=8)
        active = np.arange(npix, dtype=np.uint32)
        counts = np.zeros(npix, dtype=np.int32)
        first = rtsr.device_retire(S, Q, active, 4, 1e-3, counts)
        again = rtsr.device_retire(S, Q, active, 4, 1e-3, counts)
        assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
        walk_active = np.ones(npix, dtype=bool)
        walk_counts = np.zeros(npix, dtype=np.int32)
        for spp, q in ((2, 0.1), (3, 0.3), (5, 0.5), (8, 0.8)):
            r_all = _rel_err(S, Q, spp)
            target = float(np.quantile(r_all[walk_active], q))
            active, counts = _retire(rtsr, S, Q, active, spp, target, counts)
            retire = walk_active & (r_all <= target)
            walk_counts[retire] = spp
            walk_active &= ~retire
            assert np.array_equal(active, np.flatnonzero(walk_active)) and np.array_equal(counts, walk_counts), spp
        assert 0 < active.size < npix // 2


def _edge_moments():
    """Pixels at the rule's edges (n = SPP): zero variance, S = Q = 0 (the m + 1/256 guard), a mean of exactly -1/256 (r_c =
    +inf), negative means, NaN and +-inf in S and Q, one channel at a time and all at once."""
    nan, inf = np.nan, np.inf
    rows = [
        ([2, 2, 2], [1, 1, 1]),              # r = 0
        ([0, 0, 0], [0, 0, 0]),              # r = 0 / (1/256) = 0
        ([0, 0, 0], [1, 1, 1]),              # m = 0: r = sqrt(1/12) * 256
        ([-4 / 256, 2, 2], [1, 1, 1]),       # m + 1/256 = 0: r_0 = +inf
        ([-8, -8, -8], [20, 20, 20]),        # negative m: every r_c < 0, r = 0
        ([nan, nan, nan], [1, 1, 1]),        # all-NaN S: every r_c NaN, r = 0 (retires)
        ([2, 2, 2], [nan, nan, nan]),        # all-NaN Q: r = 0
        ([nan, 2, 2], [1, 1, 4]),            # one NaN channel ignored: r = r_2
        ([2, nan, 2], [4, nan, 1]),          # r = r_0
        ([inf, 2, 2], [1, 1, 1]),            # S = inf: var = 0, r_0 = 0
        ([2, 2, 2], [inf, 1, 1]),            # Q = inf: r_0 = inf
        ([inf, inf, inf], [inf, inf, inf]),  # inf - inf = NaN variance -> 0, r = 0
        ([-inf, 2, 2], [1, 1, 1]),           # S = -inf: r_0 = -0 / ... , r = 0
        ([2, 2, 2], [-inf, -inf, -inf]),     # var -inf -> 0: r = 0
    ]
    S = np.array([a for a, _ in rows], dtype=np.float64)
    Q = np.array([b for _, b in rows], dtype=np.float64)
    return S, Q


def test_retire_edges_and_nan_rule(rtsr):
    S, Q = _edge_moments()
    with np.errstate(invalid="ignore", divide="ignore"):
        r = _rel_err(S, Q, SPP)
    assert not np.isnan(r).any() and r[3] == np.inf and r[10] == np.inf
    assert (r[[0, 1, 4, 5, 6, 9, 11, 12, 13]] == 0.0).all()
    npix = S.shape[0]
    active = np.arange(npix, dtype=np.uint32)
    for target in (0.0, 0.5, 1e300, np.inf):
        nxt, counts = _retire(rtsr, S, Q, active, SPP, target, np.zeros(npix, dtype=np.int32))
        assert counts[5] == counts[6] == SPP, target  # the NaN rule: an all-NaN pixel retires at the first check
    # several hundred copies so the edges fall on every lane and across blocks
    reps = 300
    S2, Q2 = np.tile(S, (reps, 1)), np.tile(Q, (reps, 1))
    _retire(rtsr, S2, Q2, np.arange(S2.shape[0], dtype=np.uint32), SPP, 0.5, np.zeros(S2.shape[0], dtype=np.int32))
    _reduce(rtsr, S, Q, SPP, 0.5)
    _reduce(rtsr, S2, Q2, SPP, 0.5)
    finite = np.isfinite(r)
    got, _ = _reduce(rtsr, np.tile(S[finite], (reps, 1)), np.tile(Q[finite], (reps, 1)), SPP, 0.5)
    assert np.isfinite(got[1]) and got[1] > 0.0


def test_retire_ties(rtsr):
    """r == target retires; the next double above r stays active at a target just below it."""
    rng = np.random.default_rng(11)
    npix = 70001
    S, Q = _random_moments(npix, rng)
    r = _rel_err(S, Q, SPP)
    active = np.arange(npix, dtype=np.uint32)
    for k in (0, 63, 64, 255, 256, 40000, npix - 1):
        for target in (r[k], np.nextafter(r[k], np.inf), np.nextafter(r[k], -np.inf)):
            nxt, counts = _retire(rtsr, S, Q, active, SPP, float(target), np.zeros(npix, dtype=np.int32))
            assert (counts[k] == SPP) == (r[k] <= target), (k, target)
    # target 0 retires exactly the zero-variance pixels
    zero = rng.random(npix) < 0.3
    S[zero] = 2.0
    Q[zero] = 1.0
    r = _rel_err(S, Q, SPP)
    assert np.array_equal(r == 0.0, zero)
    nxt, counts = _retire(rtsr, S, Q, active, SPP, 0.0, np.zeros(npix, dtype=np.int32))
    assert np.array_equal(counts == SPP, zero) and np.array_equal(nxt, np.flatnonzero(~zero))


@pytest.mark.parametrize("npix", SIZES)
def test_noise_reduce_is_the_documented_tree(rtsr, npix):
    rng = np.random.default_rng(20 + npix)
    S, Q = _random_moments(npix, rng)
    for target in (0.0, 1e-3, 1.0):
        _reduce(rtsr, S, Q, SPP, target)
    # with counts: 0 = still active (at spp), the others retired at several n_p
    counts = rng.choice(np.array([0, 0, 2, 3, 5, 9], dtype=np.int32), npix)
    got, r = _reduce(rtsr, S, Q, 12, 1e-3, counts)
    again = rtsr.device_noise_reduce(S, Q, 12, 1e-3, counts)
    assert np.array(got).tobytes() == np.array(again).tobytes()
    # keep-pattern data: only exact zeros and one repeated value
    keep = _pattern("one_wave", npix, rng)
    S, Q = _keep_moments(keep)
    got, _ = _reduce(rtsr, S, Q, SPP, TARGET)
    assert got[2] == int(keep.sum())


def test_exact_sum_differs_from_numpy_sum(rtsr):
    """The bit-exact assertion has teeth: on r spanning many decades, np.sum's order gives other bits than the device tree,
    and the device agrees with the tree."""
    rng = np.random.default_rng(5)
    S, Q = _random_moments(1000000, rng)
    r = _rel_err(S, Q, SPP)
    ref = _noise_tree(r, 0.1)
    assert float(np.sum(r)) != ref.sum and float(r.cumsum()[-1]) != ref.sum
    assert rtsr.device_noise_reduce(S, Q, SPP, 0.1)[1] == ref.sum
