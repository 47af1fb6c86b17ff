"""Plain numpy references for the quantification kernels (skm_em.hip), written from
the algorithms their comments state.  Nothing here imports seekmer_amd: the tests
hold the kernels against these, and test_quant_reference.py holds these against
first principles."""
import numpy as np

M64 = (1 << 64) - 1
MN_TILES = 4096
_U32 = np.uint64(0xFFFFFFFF)
_GOLDEN = 0x9E3779B97F4A7C15          # MnStream: stream id
_PART = 0xC2B2AE3D27D4EB4F            # MnStream: part (0 = stage 1, 1 + tile = stage 2)
_SPARE = 0xA0761D6478BD642F           # MnStream: key of the redraws
_PAIR = 0xD1342543DE82EF95            # hash number of a draw pair
_ATTEMPT = 0x9FB21C651E98DF25         # redraw (2 attempt + which)


def mix64(z):
    """SplitMix64's finaliser; a Python int gives an int, an array gives uint64 (mod 2^64)."""
    if isinstance(z, (int, np.integer)):
        z = int(z) & M64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        return z ^ (z >> 31)
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over='ignore'):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def multinomial_tile(n_classes):
    tile = 1
    while (n_classes + tile - 1) // tile > MN_TILES:
        tile <<= 1
    return tile


def _uniform_draws(n, range_, seed, stream_id, part):
    """For every stream k, n[k] exactly uniform integers in [0, range_[k]) of the stream keyed
    (seed, stream_id, part[k]): draw 2p is the high word of the stream's hash number p, draw
    2p + 1 its low word; a word is turned into a draw by multiply-high with rejection
    (reject_below = 2^32 mod range), and a rejected word is replaced from the stream's redraw key
    and (pair, which, attempt).  Returns (draws, the stream of each draw, number of redraws)."""
    n = np.atleast_1d(np.asarray(n, dtype=np.int64))
    range_ = np.atleast_1d(np.asarray(range_, dtype=np.uint64))
    part = np.atleast_1d(np.asarray(part, dtype=np.uint64))
    with np.errstate(over='ignore'):
        base = mix64(np.uint64(seed & M64) ^ np.uint64((stream_id * _GOLDEN) & M64) ^ (part * np.uint64(_PART)))
    spare = mix64(base ^ np.uint64(_SPARE))
    n_pairs, n_second = (n + 1) >> 1, n >> 1
    pair_start = np.concatenate([[0], np.cumsum(n_pairs)[:-1]])
    first = np.repeat(np.arange(n.size), n_pairs)
    second = np.repeat(np.arange(n.size), n_second)
    pair = np.arange(first.size) - pair_start[first]
    pair2 = np.arange(second.size) - np.repeat(np.cumsum(n_second) - n_second, n_second)
    with np.errstate(over='ignore'):
        w = mix64(base[first] + pair.astype(np.uint64) * np.uint64(_PAIR))
    stream = np.concatenate([first, second])
    pair = np.concatenate([pair, pair2]).astype(np.uint64)
    which = np.concatenate([np.zeros(first.size, np.uint64), np.ones(second.size, np.uint64)])
    word = np.concatenate([w >> np.uint64(32), w[pair_start[second] + pair2] & _U32])
    rng = range_[stream]
    reject_below = (np.uint64(1 << 32) % range_)[stream]
    m = word * rng
    bad = np.flatnonzero((m & _U32) < reject_below)
    redraws, attempt = 0, 1
    while bad.size:
        redraws += bad.size
        with np.errstate(over='ignore'):
            key = spare[stream[bad]] + pair[bad] * np.uint64(_PAIR) \
                + (np.uint64(2 * attempt) + which[bad]) * np.uint64(_ATTEMPT)
        m[bad] = (mix64(key) >> np.uint64(32)) * rng[bad]
        bad = bad[(m[bad] & _U32) < reject_below[bad]]
        attempt += 1
    return m >> np.uint64(32), stream, redraws


def draw_counts(cum, n_draws, seed, number):
    """The bootstrap draw of skm_em.hip (multinomial_tiles_kernel + multinomial_classes_kernel)
    over ascending integer cumulative counts `cum` (internal class order), replicate `number`:
    stage 1 (stream part 0) sorts n_draws draws into tiles of multinomial_tile(C) classes by the
    tiles' cumulative counts, stage 2 (part 1 + tile) draws each tile's share among its classes
    by the cumulative counts relative to the tile; a draw r falls in the first interval whose
    cumulative count exceeds r.  Returns (counts in the order of cum, redraws taken)."""
    cum = np.asarray(cum, dtype=np.uint64)
    C = cum.size
    if C == 0 or n_draws == 0:
        return np.zeros(C, dtype=np.int64), 0
    assert n_draws < (1 << 32) and int(cum[-1]) == n_draws
    tile = multinomial_tile(C)
    n_tiles = (C + tile - 1) // tile
    tile_cum = cum[np.minimum(C, (np.arange(n_tiles) + 1) * tile) - 1]
    r, _, redraws = _uniform_draws(n_draws, tile_cum[-1], seed, number, 0)
    tile_total = np.bincount(np.searchsorted(tile_cum, r, side='right'), minlength=n_tiles)
    live = np.flatnonzero(tile_total)
    before = np.where(live > 0, cum[np.maximum(live * tile - 1, 0)], np.uint64(0)).astype(np.uint64)
    mass = tile_cum[live] - before
    r, stream, more = _uniform_draws(tile_total[live], mass, seed, number, 1 + live)
    # (the first class whose cumulative count exceeds before + r lies in the tile: the tile's
    # classes are exactly those with cum in (before, before + mass])
    cls = np.searchsorted(cum, before[stream] + r, side='right')
    return np.bincount(cls, minlength=C).astype(np.int64), redraws + more


def internal_order(offsets, targets):
    """Caller class index of internal class k: classes stably sorted by their smallest
    transcript id (skm_quant_setup.hip's locality order)."""
    offsets = np.asarray(offsets, dtype=np.int64)
    if offsets.size <= 1:
        return np.zeros(0, dtype=np.int64)
    assert (np.diff(offsets) > 0).all(), 'empty tuples'
    key = np.minimum.reduceat(np.asarray(targets, dtype=np.int64)[:offsets[-1]], offsets[:-1])
    return np.argsort(key, kind='stable')


def em_step_ld(x, l, offsets, targets, counts):
    """One step of seekmer/infer.py's EM (inner_c = sum of x over tuple c / count_c;
    x'_t = sum over t's entries of x_t / inner_c, / l_t / n; NaN -> 0) in np.longdouble.
    Returns (x', bound): bound_t = 2 (D_t + L_t + 4) 2^-53, D_t = t's (class, t) entries,
    L_t = the longest tuple among t's classes -- a first-order bound on the relative error
    of a float64 evaluation in any association (all terms >= 0)."""
    x = np.asarray(x, dtype='f8')
    offsets = np.asarray(offsets, dtype=np.int64)
    targets = np.asarray(targets, dtype=np.int64)[:offsets[-1]]
    counts = np.asarray(counts, dtype='f8')
    n_tx, C = x.size, offsets.size - 1
    lens = np.diff(offsets)
    assert (lens > 0).all(), 'empty tuples'
    cls = np.repeat(np.arange(C), lens)
    xl = x.astype(np.longdouble)
    n = np.longdouble(float(counts.sum()))
    with np.errstate(divide='ignore', invalid='ignore'):
        inner = np.add.reduceat(xl[targets], offsets[:-1]) / counts.astype(np.longdouble)
        terms = xl[targets] / inner[cls]
    order = np.argsort(targets, kind='stable')
    tx_sorted = targets[order]
    acc = np.zeros(n_tx, dtype=np.longdouble)
    if order.size:
        starts = np.flatnonzero(np.r_[True, tx_sorted[1:] != tx_sorted[:-1]])
        acc[tx_sorted[starts]] = np.add.reduceat(terms[order], starts)
    with np.errstate(divide='ignore', invalid='ignore'):
        new = acc / np.asarray(l, dtype='f8').astype(np.longdouble) / n
    new[new != new] = 0
    D = np.bincount(targets, minlength=n_tx)
    L = np.zeros(n_tx, dtype=np.int64)
    np.maximum.at(L, targets, lens[cls])
    return new, 2.0 * (D + L + 4) * 2.0 ** -53


def check_multinomial_dispersion(counts, class_count):
    """Second moments of B draws of multinomial(n, p = class_count / n) (mean AND
    variance): per class the sample variance over the replicates against n p (1 - p), and
    Pearson's statistic sum_c (x_c - n p_c)^2 / (n p_c) of every replicate, which is
    chi-square with C' - 1 degrees of freedom (C' = classes with p > 0).  Bounds are 6 sigma of
    the respective sampling distributions, so a correct generator fails with p < 1e-8."""
    counts = np.asarray(counts, dtype='f8')
    n_boot = counts.shape[0]
    n = class_count.sum()
    p = class_count / n
    live = p > 0
    assert (counts[:, ~live] == 0).all()
    var = counts[:, live].var(axis=0, ddof=1)
    expect = n * p[live] * (1 - p[live])
    big = expect > 25                                  # near-normal cells: var * (B-1) / expect ~ chi2(B-1)
    ratio = var[big] / expect[big]
    tol = 6 * np.sqrt(2.0 / (n_boot - 1))
    assert big.sum() > 0 and (np.abs(ratio - 1) < tol + 0.05).all(), (ratio.min(), ratio.max(), tol)
    # pooled: the mean of the ratios is far tighter than any single one
    assert abs(ratio.mean() - 1) < 6 * np.sqrt(2.0 / (n_boot - 1) / big.sum()) + 0.01
    cells = n * p >= 5                                 # chi-square approximation holds cell by cell
    dof = int(cells.sum()) - (1 if cells.all() else 0)
    pearson = (((counts[:, cells] - n * p[cells]) ** 2) / (n * p[cells])).sum(axis=1)
    if dof > 30:
        assert (np.abs(pearson - dof) < 6 * np.sqrt(2.0 * dof)).all(), (pearson.min(), pearson.max(), dof)
        assert abs(pearson.mean() - dof) < 6 * np.sqrt(2.0 * dof / n_boot) + 0.002 * dof
    # negative covariance between classes (-n p_i p_j): the two largest classes
    i, j = np.argsort(p)[-2:]
    cov = np.cov(counts[:, i], counts[:, j])[0, 1]
    sd = np.sqrt(n * p[i] * (1 - p[i]) * n * p[j] * (1 - p[j]) / n_boot)
    assert abs(cov + n * p[i] * p[j]) < 6 * sd * np.sqrt(2)
