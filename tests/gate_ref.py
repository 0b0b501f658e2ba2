"""NumPy int64 reference of the power gate and the window extraction on int16 rows (include/mfcc_hip.h:
mfcc_hip_gate_dev / mfcc_hip_gate_windows_dev / mfcc_hip_gate_*).  Test infrastructure only; written from the header's
description and the behaviour of the receiver's loop, software/cepstrum.c:161-183."""
import numpy as np

POWER_THRESHOLD = 100000000


def windows_of(T, n_frames, stride):
    """Windows of a segment of T rows."""
    return (T - n_frames) // stride + 1 if T >= n_frames else 0


def loop_elements(n_cep, n_frames):
    """The flat indices the receiver's loop visits on a linear window (head = 0)."""
    size = n_frames * n_cep
    return list(range(size // 3, 2 * size // 3, n_cep))


def geometry(n_cep, n_frames):
    """(K, f0, c0): the loop's elements are column c0 of frames f0 .. f0 + K - 1."""
    size = n_frames * n_cep
    first, last = size // 3, 2 * size // 3
    return -(-(last - first) // n_cep), first // n_cep, first % n_cep


def wrap32(power):
    """An int64 sum as a 32-bit two's-complement int holds it."""
    return (np.asarray(power, dtype=np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32) \
        .astype(np.int64)


def win_offsets(offsets, n_frames, stride):
    offsets = np.asarray(offsets, dtype=np.int64)
    wo = np.zeros(len(offsets), dtype=np.int64)
    for k in range(len(offsets) - 1):
        wo[k + 1] = wo[k] + windows_of(int(offsets[k + 1] - offsets[k]), n_frames, stride)
    return wo


def gate(rows, offsets, n_frames, stride, threshold=POWER_THRESHOLD):
    """rows int16 (R, n_cep), segment k = rows offsets[k]:offsets[k + 1] -> (power int64, gate uint8, gate_ref uint8,
    win_offsets), one entry per window in segment order."""
    rows = np.asarray(rows)
    assert rows.dtype == np.int16 and rows.ndim == 2
    n_cep = rows.shape[1]
    K, f0, c0 = geometry(n_cep, n_frames)
    wo = win_offsets(offsets, n_frames, stride)
    power = np.zeros(int(wo[-1]), dtype=np.int64)
    sq = rows[:, c0].astype(np.int64) ** 2 if rows.shape[0] else np.zeros(0, dtype=np.int64)
    pre = np.concatenate([[0], np.cumsum(sq)])
    for k in range(len(offsets) - 1):
        nw = int(wo[k + 1] - wo[k])
        if nw:
            a = int(offsets[k]) + f0 + np.arange(nw, dtype=np.int64) * stride
            power[wo[k]:wo[k + 1]] = pre[a + K] - pre[a]
    return power, (power >= threshold).astype(np.uint8), (wrap32(power) >= threshold).astype(np.uint8), wo


def starts_of(offsets, n_frames, stride):
    """First row (index into rows) of every window, in the order of gate()'s outputs."""
    out = []
    for k in range(len(offsets) - 1):
        nw = windows_of(int(offsets[k + 1] - offsets[k]), n_frames, stride)
        out.append(int(offsets[k]) + np.arange(nw, dtype=np.int64) * stride)
    return np.concatenate(out) if out else np.zeros(0, dtype=np.int64)


def take(rows, offsets, mask, n_frames, stride):
    """(windows (n, n_frames, n_cep), starts int64, out_offsets) of the windows whose mask byte is not 0."""
    rows = np.asarray(rows)
    mask = np.asarray(mask)
    st = starts_of(offsets, n_frames, stride)
    assert len(st) == len(mask)
    wo = win_offsets(offsets, n_frames, stride)
    keep = mask != 0
    sel = st[keep]
    wins = np.stack([rows[s:s + n_frames] for s in sel]) if len(sel) else \
        np.zeros((0, n_frames, rows.shape[1]), dtype=np.int16)
    oo = np.concatenate([[0], np.cumsum(keep)])[wo]
    return wins, sel, oo.astype(np.int64)


class Tracker:
    """Line-by-line model of the gate tracker: every line keeps ALL its rows since create / reset."""

    def __init__(self, n_lines, n_cep, n_frames, stride, threshold=POWER_THRESHOLD):
        self.n_lines, self.n_cep, self.n_frames, self.stride, self.threshold = n_lines, n_cep, n_frames, stride, threshold
        self.rows = [np.zeros((0, n_cep), dtype=np.int16) for _ in range(n_lines)]

    @property
    def seen(self):
        return np.array([len(r) for r in self.rows], dtype=np.int64)

    def plan(self, lengths):
        """win_offsets of a push of these many new rows per line."""
        wo = np.zeros(self.n_lines + 1, dtype=np.int64)
        for u, nf in enumerate(lengths):
            s = len(self.rows[u])
            # the windows j with s <= j * stride + n_frames - 1 < s + nf
            n = sum(1 for j in range(windows_of(s + int(nf), self.n_frames, self.stride))
                    if j * self.stride + self.n_frames - 1 >= s)
            wo[u + 1] = wo[u] + n
        return wo

    def push(self, chunks):
        """chunks: one (nf, n_cep) int16 array per line -> (power, gate, gate_ref, win_offsets) of the completed windows."""
        wo = self.plan([len(c) for c in chunks])
        P, G, R = [], [], []
        for u, c in enumerate(chunks):
            before = windows_of(len(self.rows[u]), self.n_frames, self.stride)
            self.rows[u] = np.concatenate([self.rows[u], np.asarray(c, dtype=np.int16).reshape(-1, self.n_cep)])
            p, g, r, _ = gate(self.rows[u], [0, len(self.rows[u])], self.n_frames, self.stride, self.threshold)
            P.append(p[before:])
            G.append(g[before:])
            R.append(r[before:])
            assert len(p) - before == wo[u + 1] - wo[u]
        return np.concatenate(P), np.concatenate(G), np.concatenate(R), wo

    def reset(self, lines=None):
        for u in (range(self.n_lines) if lines is None else lines):
            self.rows[u] = np.zeros((0, self.n_cep), dtype=np.int16)

    def last_window(self, u):
        nw = windows_of(len(self.rows[u]), self.n_frames, self.stride)
        assert nw > 0
        s = (nw - 1) * self.stride
        return self.rows[u][s:s + self.n_frames]
