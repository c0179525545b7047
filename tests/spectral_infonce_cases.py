"""Seeded inputs and a numpy restatement of the cross-patch negatives and the pair-similarity statistics of the global spectral InfoNCE
(frl/training/representation/step.py:743-773 and :798-807), written from the formulas:

  blocks      the ordered patch pairs (pi, pj), pi != pj, in the reference's loop order (pi outer, pj inner): block b has pi = b // (S - 1),
              r = b % (S - 1), pj = r + (r >= pi).  Each block holds n_per = max(1, neg_per_anchor * N // (S (S - 1))) negatives.
  picks       negative q of block b = q // n_per takes i = offsets[pi] + ((draws[q][0] * count_pi) >> 31) and
              j = offsets[pj] + ((draws[q][1] * count_pj) >> 31), draws in [0, 2^31).
  weights     d = |spec[i] - spec[j]|_2 and clamp(1 - exp(-d / tau), min_w, 1), in float64.
  sims        -|z[a] - z[b]|^2 / D in float64; mean and unbiased standard deviation.

Case table (tests/golden/spectral_infonce_{a,b,c,d}.npz hold the expected outputs, written by tests/golden/make_spectral_infonce_golden.py
with the reference's pairs_mutual_knn_chunked and contrastive_loss; the inputs come from the seeds below).  A case's seed is the first of
0..31 at which the reference's mutual-kNN list is the same in float32 and float64 and the k + 1 nearest distances of every row are at least
1e-5 apart (relative): the maker asserts that.
"""
import numpy as np

CASES = {
    "a": dict(patches=(12, 30, 25), C=7, D=16, k=4, neg_per_anchor=20, seed=0),
    "b": dict(patches=(1, 7, 40), C=33, D=64, k=4, neg_per_anchor=3, seed=0),             # a single-anchor patch, n_per = 24
    "c": dict(patches=(40, 40), C=1, D=8, k=8, neg_per_anchor=20, seed=0),                # C = 1: weights on the min_w clamp
    "d": dict(patches=(9, 17, 23, 5, 31), C=16, D=64, k=16, neg_per_anchor=1, seed=2),    # n_per = 4, 16-byte rows; seeds 0 and 1 have
}                                                                                         # two neighbours less than 1e-5 apart
MIN_SPATIAL, GRID, TAU, MIN_W, TEMPERATURE = 4.0, 32, 1.0, 0.05, 0.07
DRAW_TOP = 2 ** 31 - 1


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------

def offsets_of(patches):
    return [0] + np.cumsum(patches).tolist()


def n_per_of(neg_per_anchor, n, s):
    pairs = s * (s - 1)
    return max(1, (neg_per_anchor * n) // pairs) if pairs > 0 else 0


def make_draws(q, seed):
    """int64 [q, 2] in [0, 2^31); the first row is (0, 0) and the second (2^31 - 1, 2^31 - 1)."""
    d = np.random.default_rng(seed).integers(0, 2 ** 31, (q, 2)).astype(np.int64)
    if q > 0:
        d[0] = 0
    if q > 1:
        d[1] = DRAW_TOP
    return d


def make_rows(n, width, seed):
    """float32 [n, width], unit-variance normal."""
    return np.random.default_rng(seed).standard_normal((n, width)).astype(np.float32)


def make_inputs(name, seed=None):
    """-> dict(spec [N, C] f32, z [N, D] f32, coords (list of int64 [n_p, 2]), offsets (list), n_per, draws int64 [Q, 2])."""
    c = CASES[name]
    seed = c["seed"] if seed is None else seed
    base = 1000 * (ord(name) - ord("a") + 1) + 10 * seed
    offsets = offsets_of(c["patches"])
    n, s = offsets[-1], len(c["patches"])
    rng = np.random.default_rng(base + 2)
    coords = [rng.integers(0, GRID, (m, 2)).astype(np.int64) for m in c["patches"]]
    n_per = n_per_of(c["neg_per_anchor"], n, s)
    return dict(spec=make_rows(n, c["C"], base), z=make_rows(n, c["D"], base + 1), coords=coords, offsets=offsets, n_per=n_per,
                draws=make_draws(n_per * s * (s - 1), base + 3))


# ---- restatement ----------------------------------------------------------------------------------------------------------------------

def blocks(s):
    """[(pi, pj)] for b = 0 .. s (s - 1) - 1 by the arithmetic rule."""
    out = []
    for b in range(s * (s - 1)):
        pi, r = b // (s - 1), b % (s - 1)
        out.append((pi, r + (1 if r >= pi else 0)))
    return out


def pick(draw, lo, hi):
    return lo + ((int(draw) * (hi - lo)) >> 31)


def negative_pairs(offsets, n_per, draws):
    """-> int64 [Q, 2]; `pick` for every negative, as array arithmetic (draw * count < 2^62)."""
    s = len(offsets) - 1
    offs = np.asarray(offsets, dtype=np.int64)
    patch = np.repeat(np.asarray(blocks(s), dtype=np.int64).reshape(-1, 2), n_per, axis=0)            # [Q, 2] = (pi, pj) of every negative
    draws = np.asarray(draws, dtype=np.int64).reshape(-1, 2)
    assert draws.shape == patch.shape and (draws >= 0).all() and (draws < 2 ** 31).all()
    return offs[patch] + ((draws * (offs[patch + 1] - offs[patch])) >> 31)


def distances(spec, pairs):
    x = np.asarray(spec, dtype=np.float64)
    return np.sqrt(((x[pairs[:, 0]] - x[pairs[:, 1]]) ** 2).sum(axis=1))


def weights(dist, tau=TAU, min_w=MIN_W):
    return np.clip(1.0 - np.exp(-np.asarray(dist, dtype=np.float64) / tau), min_w, 1.0)


def negatives(spec, offsets, n_per, draws, tau=TAU, min_w=MIN_W):
    """-> (pairs int64 [Q, 2], dist float64 [Q], weights float64 [Q])."""
    pairs = negative_pairs(offsets, n_per, draws)
    dist = distances(spec, pairs)
    return pairs, dist, weights(dist, tau, min_w)


def sims(z, pairs):
    x = np.asarray(z, dtype=np.float64)
    return -((x[pairs[:, 0]] - x[pairs[:, 1]]) ** 2).sum(axis=1) / x.shape[1]


def sim_stats(z, pairs):
    """-> (mean, unbiased standard deviation) in float64; the deviation of fewer than two values is NaN."""
    v = sims(z, pairs)
    return float(v.mean()), float(v.std(ddof=1)) if len(v) > 1 else float("nan")
