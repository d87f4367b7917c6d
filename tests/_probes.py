"""Helpers of tests/test_wide_probes_{cpu,gpu}.py: a NumPy restatement of the library's Philox4x32-10 and of the
Rademacher draw built on it (pita_amd/csrc/common.h: Philox, philox_rademacher_word, rademacher_sign), and the fp64
quadratic forms of the Hutchinson estimator on an oracle Jacobian."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c, seed):
    """c: four uint64 arrays holding 32-bit counter words, seed: 64-bit int -> the four output words (Philox::gen)."""
    c = [np.asarray(v, dtype=np.uint64) & MASK32 for v in c]
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]  # 32 x 32 -> 64 bit, no overflow
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0)) & MASK32, p1 & MASK32,
             ((p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1)) & MASK32, p0 & MASK32]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def rademacher_probes(B, n, d, K, seed=0, walker_offset=0, step=0):
    """[K, B, n*d] float32 of +1 / -1: counter (walker lo, walker hi, step lo, tag ^ (step hi << 20)) with
    tag = 0x80000 | (probe << 10) | particle, coordinate k = bit k of the first output word."""
    k, b, i = np.meshgrid(np.arange(K, dtype=np.uint64), np.arange(B, dtype=np.uint64), np.arange(n, dtype=np.uint64),
                          indexing="ij")
    walker = (b + np.uint64(walker_offset & 0xFFFFFFFFFFFFFFFF))  # wraps like the kernel's 64-bit add
    step64 = step & 0xFFFFFFFFFFFFFFFF
    tag = (np.uint64(0x80000) | (k << np.uint64(10)) | i) ^ np.uint64(((step64 >> 32) << 20) & 0xFFFFFFFF)
    word = philox4x32_10([walker & MASK32, walker >> np.uint64(32), np.full_like(k, step64 & 0xFFFFFFFF), tag],
                         seed & 0xFFFFFFFFFFFFFFFF)[0]
    bits = (word[..., None] >> np.arange(d, dtype=np.uint64)) & np.uint64(1)
    return np.where(bits == 1, 1.0, -1.0).astype(np.float32).reshape(K, B, n * d)


def quadratic_forms(J, V):
    """J [B, D, D] float64, V [K, B, D] -> (q [K, B] = v^T J v, l1 [K, B] = sum_i |(J v)_i|), float64."""
    J, V = np.asarray(J, dtype=np.float64), np.asarray(V, dtype=np.float64)
    Jv = np.einsum("bij,kbj->kbi", J, V)
    return np.einsum("kbi,kbi->kb", V, Jv), np.abs(Jv).sum(-1)


def rademacher_sigma(J):
    """One-probe standard deviation of v^T J v under Rademacher v: sqrt(1/2 sum_{i != j} (J_ij + J_ji)^2), [B]."""
    J = np.asarray(J, dtype=np.float64)
    S = J + np.swapaxes(J, 1, 2)
    off = S - np.einsum("bii->bi", S)[:, :, None] * np.eye(S.shape[1])
    return np.sqrt(0.5 * (off ** 2).sum((1, 2)))


def fp32_mean(q):
    """The library's final reduction in NumPy float32: sum over k from +0 in probe order, divided by (float)K."""
    q = np.asarray(q, dtype=np.float32)
    s = np.zeros(q.shape[1], dtype=np.float32)
    for k in range(q.shape[0]):
        s = (s + q[k]).astype(np.float32)
    return (s / np.float32(q.shape[0])).astype(np.float32)
