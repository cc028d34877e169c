"""The evolutionary search's device primitives restated in numpy (fp64): Philox4x32-10, the sampler (ias_evolve_sample),
the running top-k (ias_topk_merge) and the distribution update (ias_evolve_update), as include/ias_hip.h specifies them,
and the three as ``evolve.cross_entropy_search``'s ``ops`` on CPU tensors.  Test support: no test lives here."""
from types import SimpleNamespace

import numpy as np
import torch

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
EMPTY = np.iinfo(np.int64).max


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints) of one shape, key: two ints -> four uint64 arrays holding 32-bit words."""
    c = [np.asarray(x, dtype=np.uint64) & np.uint64(MASK) for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]                          # < 2^64: both factors are below 2^32
        p1 = np.uint64(M1) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(MASK)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def unit(x):
    """u(x) = ((x >> 9) + 0.5) 2^-23 in (0, 1), exact in fp32 and fp64."""
    return ((np.asarray(x, dtype=np.uint64) >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def normals(N, M, P, n_base, m_base, seed, generation):
    """z [N, M, P] fp64: the standard normals of ias_evolve_sample, counter (m', n', generation, j >> 2)."""
    G = (P + 3) // 4
    n = (n_base + np.arange(N, dtype=np.uint64)).reshape(N, 1, 1)
    m = (m_base + np.arange(M, dtype=np.uint64)).reshape(1, M, 1)
    q = np.arange(G, dtype=np.uint64).reshape(1, 1, G)
    gen = np.full((1, 1, 1), generation, dtype=np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    x = philox4x32_10((m, n, gen, q), (seed & MASK, seed >> 32))
    z = np.empty((N, M, G, 4))
    for a in (0, 2):
        r = np.sqrt(-2.0 * np.log(unit(x[a])))
        t = 2.0 * np.pi * unit(x[a + 1])
        z[..., a] = r * np.cos(t)
        z[..., a + 1] = r * np.sin(t)
    return z.reshape(N, M, 4 * G)[:, :, :P]


def sample(mean, sigma, free, M, n_base=0, m_base=0, seed=0, generation=0):
    """mean, sigma [N, P] (fp32 values), free [P] -> out [N, M, P] fp64 (the fp32 kernel rounds the product and the sum)."""
    mean, sigma = np.asarray(mean, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
    N, P = mean.shape
    z = normals(N, M, P, n_base, m_base, seed, generation)
    out = np.clip(mean[:, None, :] + sigma[:, None, :] * z, 0.0, 1.0)
    return np.where(np.asarray(free, dtype=bool)[None, None, :], out, mean[:, None, :])


def merge(dist, base, best_dist, best_idx):
    """ias_topk_merge on arrays: -> (best_dist, best_idx) [N, k] after merging the block."""
    dist, best_dist, best_idx = np.asarray(dist), np.asarray(best_dist), np.asarray(best_idx)
    N, M = dist.shape
    k = best_dist.shape[1]
    d = np.concatenate([best_dist, dist], axis=1)
    ix = np.concatenate([best_idx, np.broadcast_to(base + np.arange(M, dtype=np.int64), (N, M))], axis=1)
    key = np.where(np.isfinite(d), d, np.inf)
    od, oi = np.empty_like(best_dist), np.empty_like(best_idx)
    for n in range(N):
        order = np.lexsort((ix[n], key[n]))[:k]
        od[n], oi[n] = d[n, order], ix[n, order]
    return od, oi


def update(pop, base, elite_dist, elite_idx, prev_idx, prev_params, mean, sigma, free, alpha, sigma_min, sigma_max):
    """-> (elite_params [N, k, P] fp32, mean [N, P] fp32, sigma [N, P] fp32) as ias_evolve_update leaves them."""
    pop, prev_params = np.asarray(pop, dtype=np.float32), np.asarray(prev_params, dtype=np.float32)
    mean, sigma = np.array(mean, dtype=np.float32), np.array(sigma, dtype=np.float32)
    N, M, P = pop.shape
    k = elite_idx.shape[1]
    ep = np.empty((N, k, P), dtype=np.float32)
    for n in range(N):
        valid = []
        for e in range(k):
            ix = int(elite_idx[n, e])
            if ix == EMPTY:
                ep[n, e] = 0.0
            elif base <= ix < base + M:
                ep[n, e] = pop[n, ix - base]
            else:
                hit = [s for s in range(k) if int(prev_idx[n, s]) == ix]
                ep[n, e] = prev_params[n, hit[0]] if hit else np.nan
            if ix != EMPTY and np.isfinite(elite_dist[n, e]):
                valid.append(e)
        c = len(valid)
        if c == 0:
            continue
        for j in range(P):
            if not free[j]:
                continue
            s = 0.0
            for e in valid:
                s += float(ep[n, e, j])
            mu = s / c
            v = 0.0
            for e in valid:
                d = float(ep[n, e, j]) - mu
                v += d * d
            v /= c
            with np.errstate(invalid="ignore"):
                m2 = np.clip((1.0 - alpha) * float(mean[n, j]) + alpha * mu, 0.0, 1.0)
                s2 = np.minimum(sigma_max, np.maximum(sigma_min, (1.0 - alpha) * float(sigma[n, j]) + alpha * np.sqrt(v)))
            mean[n, j], sigma[n, j] = np.float32(m2), np.float32(s2)
    return ep, mean, sigma


# ------------------------------------------------------------------ the primitives of the search loop on CPU tensors
def _sample_op(mean, sigma, free, seed, generation, out):
    pop = sample(mean.numpy(), sigma.numpy(), free.numpy(), out.shape[1], seed=seed, generation=generation)
    out.copy_(torch.from_numpy(pop.astype(np.float32)))
    return out


def _merge_op(dist, base, best_dist, best_idx):
    d, i = merge(dist.numpy(), base, best_dist.numpy(), best_idx.numpy())
    best_dist.copy_(torch.from_numpy(d))
    best_idx.copy_(torch.from_numpy(i))


def _update_op(pop, base, elite_dist, elite_idx, prev_idx, prev_params, elite_params, mean, sigma, free, alpha, sigma_min,
               sigma_max):
    ep, m, s = update(pop.numpy(), base, elite_dist.numpy(), elite_idx.numpy(), prev_idx.numpy(), prev_params.numpy(),
                      mean.numpy(), sigma.numpy(), free.numpy(), alpha, sigma_min, sigma_max)
    elite_params.copy_(torch.from_numpy(ep))
    mean.copy_(torch.from_numpy(m))
    sigma.copy_(torch.from_numpy(s))


MODEL_OPS = SimpleNamespace(sample=_sample_op, merge=_merge_op, update=_update_op)
