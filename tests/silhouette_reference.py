"""The silhouette's yardstick: a long-double numpy restatement of the definition in include/mlhip.h (mlhip_silhouette), with
numpy's own summation order, and the accuracy limit the library's fixed arithmetic is held to."""
import numpy as np

U = 2.0 ** -53
CHUNK = 256          # kSilhouetteChunk (ml_amd/csrc/device/device.hpp)


def silhouette_parts(X, labels, rows=None):
    """(a, b, s) as long-double arrays for `rows` (default: all) of X (N x d) under integer `labels`: a = mean distance to the other
    rows of the own cluster (0 for a row alone in it), b = the smallest mean distance to another non-empty cluster, s = (b - a) /
    max(a, b), 0 for a row alone in its cluster and where max(a, b) = 0."""
    X = np.asarray(X, dtype=np.float64)
    labels = np.asarray(labels).astype(np.int64)
    n = len(X)
    rows = np.arange(n) if rows is None else np.asarray(rows).astype(np.int64)
    Xl = X.astype(np.longdouble)
    used = np.unique(labels)
    counts = np.array([(labels == c).sum() for c in used])
    a = np.zeros(len(rows), dtype=np.longdouble)
    b = np.zeros(len(rows), dtype=np.longdouble)
    s = np.zeros(len(rows), dtype=np.longdouble)
    for lo in range(0, len(rows), 256):
        idx = rows[lo:lo + 256]
        q = np.zeros((len(idx), n), dtype=np.longdouble)
        for j in range(X.shape[1]):
            z = Xl[idx, j][:, None] - Xl[None, :, j]
            q += z * z
        dist = np.sqrt(q)
        sums = np.stack([dist[:, labels == c].sum(axis=1) for c in used], axis=1)        # (rows, used clusters)
        for r, i in enumerate(idx):
            own = int(np.searchsorted(used, labels[i]))
            means = sums[r] / counts.astype(np.longdouble)
            others = np.delete(means, own)
            bi = others.min()
            if counts[own] == 1:
                ai, si = np.longdouble(0), np.longdouble(0)
            else:
                ai = sums[r, own] / np.longdouble(counts[own] - 1)
                top = max(ai, bi)
                si = np.longdouble(0) if top == 0 else (bi - ai) / top
            a[lo + r], b[lo + r], s[lo + r] = ai, bi, si
    return a, b, s


def silhouette_samples(X, labels, rows=None):
    return silhouette_parts(X, labels, rows)[2]


def chain_length(labels, shards=1, chunk=CHUNK):
    """L of the limit: the longest chain of additions behind a sum D_ic -- the chunk length (at most the largest cluster) plus the
    chunks of the largest cluster, plus the shard count on a device group."""
    counts = np.bincount(np.asarray(labels).astype(np.int64))
    largest = int(counts.max())
    return min(chunk, largest) + -(-largest // chunk) + (shards if shards > 1 else 0)


def silhouette_limit(d, L):
    """(E, limit of |s^ - s|, relative limit of a and b) for dimension d and chain length L:
    E = ((d + 2) / 2 + 2 + L) u bounds the relative error of a sum D_ic of non-negative terms; a and b add one division each
    (E + 2 u with the slack for second-order terms); s = (b - a) / max(a, b) with |s| <= 1: 3 E + 3 u."""
    E = ((d + 2) / 2 + 2 + L) * U
    return E, 3 * E + 3 * U, E + 2 * U


def worst_ratios(got_a, got_b, got_s, ref, d, L):
    """The largest errors of (a, b, s) as fractions of their limits (each must be <= 1)."""
    ra, rb, rs = ref
    _, s_lim, ab_lim = silhouette_limit(d, L)

    def rel(got, want):
        got = np.asarray(got).astype(np.longdouble)
        scale = np.where(want == 0, np.longdouble(1), np.abs(want))
        return float(np.max(np.abs(got - want) / scale)) if len(want) else 0.0
    err_s = float(np.max(np.abs(np.asarray(got_s).astype(np.longdouble) - rs))) if len(rs) else 0.0
    return rel(got_a, ra) / ab_lim, rel(got_b, rb) / ab_lim, err_s / s_lim
