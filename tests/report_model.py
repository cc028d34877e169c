"""The fp64 numpy model of ias_spectral_report (include/ias_hip_report.h) and the inputs of its tests.

The model takes the SAME fp32 arrays the kernel gets (values, target, floors, the fp32 DCT table), so what a test compares
is the kernel's arithmetic alone, not an STFT's rounding, and the counted-frame decision (a comparison of raw fp32 numbers)
is the kernel's own."""
import functools

import numpy as np

LOG10_2 = np.log10(2.0)

# (B, F, K, C, power): the mel shape; linear bins; rows at every 16-byte phase; K under one wave; one frame; one bin past a
# wave with F across several workgroups (chunks of 32 frames); the largest K; both dct limits (C = 32, K = 256)
CASES = [(3, 7, 128, 13, 2), (2, 5, 513, 0, 1), (3, 9, 257, 0, 1), (2, 3, 5, 3, 1), (1, 1, 64, 20, 2),
         (2, 70, 65, 32, 2), (1, 2, 2048, 0, 1), (2, 4, 256, 32, 2)]


def dct_table(n_in, n_coef):
    """D[c - 1, k] = sqrt(2 / n_in) cos(pi c (2 k + 1) / (2 n_in)), c = 1 .. n_coef, in fp64: the orthonormal DCT-II
    without its row 0."""
    c = np.arange(1, n_coef + 1, dtype=np.float64)[:, None]
    k = np.arange(n_in, dtype=np.float64)[None, :]
    return np.sqrt(2.0 / n_in) * np.cos(np.pi * c * (2.0 * k + 1.0) / (2.0 * n_in))


def counted(values, target, floor_rows):
    """[B, F] bool: the frames whose largest raw value, on either side, is above the row's floor."""
    return np.maximum(values, target).max(axis=2) > np.asarray(floor_rows)[:, None]


def clamped_share(values, target, floor_rows):
    """[B]: the share of the elements of the counted frames, both sides together, that sit under the row's floor."""
    fl = np.asarray(floor_rows)[:, None, None]
    cnt = counted(values, target, floor_rows)[:, :, None]
    under = ((values < fl) & cnt).sum(axis=(1, 2)) + ((target < fl) & cnt).sum(axis=(1, 2))
    total = 2.0 * cnt.sum(axis=(1, 2)) * values.shape[2]
    return under / np.maximum(total, 1.0)


def report(values, target, floor_rows, power, dct=None):
    """-> [B, 5] fp64 {lsd_db, spectral_convergence, log_l1_db, mcd_db, n} of fp32 values, target [B, F, K], floor_rows [B]
    and the table dct [C, K] the kernel gets (or None), everything in fp64 from there."""
    assert values.dtype == target.dtype == np.float32 and values.shape == target.shape and values.ndim == 3
    assert power in (1, 2)
    B, F, K = values.shape
    fl32 = np.asarray(floor_rows, dtype=np.float32)
    v, t = values.astype(np.float64), target.astype(np.float64)
    fl = fl32.astype(np.float64)[:, None, None]
    d = np.log2(np.maximum(v, fl)) - np.log2(np.maximum(t, fl))
    cnt = counted(values, target, fl32)
    n = cnt.sum(axis=1).astype(np.float64)
    a = (20.0 / power) * LOG10_2
    div = np.maximum(n, 1.0)                                          # n = 0: the sums are 0 as well
    out = np.zeros((B, 5))
    out[:, 0] = a * (np.sqrt((d * d).mean(axis=2)) * cnt).sum(axis=1) / div
    num, den = ((t - v) ** 2).sum(axis=(1, 2)), (t * t).sum(axis=(1, 2))
    with np.errstate(divide="ignore", invalid="ignore"):
        out[:, 1] = np.where(den > 0.0, np.sqrt(num) / np.sqrt(np.where(den > 0.0, den, 1.0)),
                             np.where(num > 0.0, np.inf, 0.0))
    out[:, 2] = a * (np.abs(d).sum(axis=2) * cnt).sum(axis=1) / (div * K)
    if dct is not None:
        D = np.asarray(dct, dtype=np.float64)
        assert D.shape[1] == K
        m = np.einsum("ck,bfk->bfc", D, (np.log(2.0) / power) * d)
        out[:, 3] = (10.0 / np.log(10.0)) * (np.sqrt(2.0 * (m * m).sum(axis=2)) * cnt).sum(axis=1) / div
    out[:, 4] = n
    return out


@functools.lru_cache(maxsize=None)
def inputs(case):
    """-> (values, target [B, F, K] fp32, floor_rows [B] fp32) of CASES[case]: t = g^2 exp(-k / (0.3 K)),
    v = t exp(0.5 g'), g and g' standard normal, seeded per case; floor = 1e-4 rowmax(t).  Where B > 1, row 1 has v == t;
    where F > 2, frame 1 of row 0 is zero on both sides (uncounted)."""
    B, F, K, _C, _power = CASES[case]
    rng = np.random.default_rng(700 + case)
    k = np.arange(K, dtype=np.float64)
    t = rng.standard_normal((B, F, K)) ** 2 * np.exp(-k / (0.3 * K))
    v = t * np.exp(0.5 * rng.standard_normal((B, F, K)))
    t, v = t.astype(np.float32), v.astype(np.float32)
    if B > 1:
        v[1] = t[1]
    if F > 2:
        t[0, 1] = 0.0
        v[0, 1] = 0.0
    floor = (np.float32(1e-4) * t.reshape(B, -1).max(axis=1)).astype(np.float32)
    for a in (v, t, floor):
        a.setflags(write=False)
    return v, t, floor


def one_hot(F, K, f, k, ratio=16.0):
    """-> (values, target [1, F, K], floor [1]): v == t == 1 everywhere but v[0, f, k] = ratio; floor 1e-4."""
    t = np.ones((1, F, K), dtype=np.float32)
    v = t.copy()
    v[0, f, k] = ratio
    return v, t, np.full(1, 1e-4, dtype=np.float32)
