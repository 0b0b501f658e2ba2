"""The sample-rate conversion of include/mfcc_hip.h ("sample rates"), restated in NumPy, in two parts that do not
depend on each other: the float64 design of the tap table (nothing of the library in it) and the index rule, which runs
on whatever table it is given (the tests hand it the library's, read through mfcc_hip_resample_taps).  The streaming
form is simulated by brute force from the one-shot rule."""
import math

import numpy as np

Z, BETA, ROLLOFF = 16, 7.5, 0.90

# the ratios of the host and the GPU tests: (in_rate, out_rate)
RATIOS = [(8000, 16000), (48000, 16000), (44100, 16000), (16000, 8000), (11025, 16000), (48000, 44100), (7, 5), (16000, 16000)]


def geometry(in_rate, out_rate):
    """(L, M, H, K)"""
    g = math.gcd(in_rate, out_rate)
    L, M = out_rate // g, in_rate // g
    H = Z if L >= M else -(-Z * M // L)
    return L, M, H, 2 * H


def design(in_rate, out_rate):
    """the normalised float64 design, (L, K): every phase sums to 1"""
    L, M, H, K = geometry(in_rate, out_rate)
    fc = ROLLOFF * min(1.0, L / M)
    d = np.arange(K, dtype=np.float64)[None, :] - H + 1 - np.arange(L, dtype=np.float64)[:, None] / L
    r = d / H
    g = fc * np.sinc(fc * d) * np.i0(BETA * np.sqrt(np.clip(1 - r * r, 0, None))) / np.i0(BETA)
    g[np.abs(r) > 1] = 0.0
    return g / g.sum(axis=1, keepdims=True)


def count(n, L, M):
    return (n * L + M - 1) // M


def emitted(c, L, M, H):
    return count(max(c - H, 0), L, M)


def accumulate(taps, x, L, M, m0, m1):
    """the int64 sums of outputs [m0, m1) on the table `taps` (L, K): x is zero outside [0, len(x))"""
    K = taps.shape[1]
    H = K // 2
    xp = np.concatenate([np.zeros(H - 1, np.int64), np.asarray(x, np.int64), np.zeros(K + 1, np.int64)])
    out = np.empty(max(m1 - m0, 0), np.int64)
    t64 = taps.astype(np.int64)
    for a in range(m0, m1, 1 << 16):
        m = np.arange(a, min(a + (1 << 16), m1), dtype=np.int64)
        q, p = m * M // L, m * M % L
        idx = np.minimum(q[:, None] + np.arange(K)[None, :], len(xp) - 1)      # x[q - H + 1 + k] is xp[q + k]
        out[a - m0:a - m0 + len(m)] = (t64[p] * xp[idx]).sum(axis=1)
    return out


def finish(acc):
    return np.clip((acc + 8192) >> 14, -32768, 32767).astype(np.int16)


def resample(taps, x, L, M, m0=0, m1=None):
    """outputs [m0, m1) (default: all count(len(x)) of them)"""
    return finish(accumulate(taps, x, L, M, m0, count(len(x), L, M) if m1 is None else m1))


def stream(taps, chunks, L, M):
    """(what every push returns, what the flush returns): after c samples a line has emitted E(c) outputs, each
    computed by the one-shot rule on everything pushed so far -- none of them reads beyond it"""
    H = taps.shape[1] // 2
    seen, outs, done = np.zeros(0, np.int16), [], 0
    for ch in chunks:
        seen = np.concatenate([seen, np.asarray(ch, np.int16)])
        e = emitted(len(seen), L, M, H)
        outs.append(resample(taps, seen, L, M, done, e))
        done = e
    return outs, resample(taps, seen, L, M, done, count(len(seen), L, M))
