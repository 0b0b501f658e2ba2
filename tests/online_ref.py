"""Helpers of the online stream bank's GPU tests -- TEST INFRASTRUCTURE ONLY (a plain module, not a conftest): the
bank's settings and the one-shot handle they correspond to, schedules of chunk lengths, the two ways to push, and a
Python model of the plan (which rows a lagged session has returned)."""
from __future__ import annotations

import numpy as np

import kernel_families as kf

BY_ID = {f.id: f for f in kf.ALL}

# the bank's settings (MFCC.stream_bank keywords)
MEANVAR40_DD2 = dict(normalize="meanvar", normalize_window=40, deltas=2, delta_window=2)
MEAN5 = dict(normalize="mean", normalize_window=5)
RAW_D8 = dict(deltas=1, delta_window=8)
MEANVAR600_DD2 = dict(normalize="meanvar", normalize_window=600, deltas=2, delta_window=2)
SETTINGS = {"meanvar40_dd2": MEANVAR40_DD2, "mean5": MEAN5, "raw_d8": RAW_D8}


def lag_of(cfg):
    return cfg.get("deltas", 0) * cfg.get("delta_window", 2)


def one_shot_kwargs(cfg):
    """The one-shot handle an online bank with ``cfg`` is held to: the purely causal window, min_window 1."""
    kw = dict(deltas=cfg.get("deltas", 0), delta_window=cfg.get("delta_window", 2))
    if cfg.get("normalize"):
        kw.update(normalize=cfg["normalize"], normalize_window=cfg["normalize_window"], normalize_min_window=1,
                  normalize_center=False)
    return kw


def length(fam, n_frames, pad):
    """Samples that give ``n_frames`` frames in framing ``pad`` (and half a hop more for STREAM)."""
    if pad == "notebook":
        return fam.hop * (n_frames - 1) + fam.nfft
    if n_frames == 1:
        return fam.nfft // 2
    return fam.hop * (n_frames - 2) + fam.nfft + fam.hop // 2


def sizes(fam):
    hop, nfft = fam.hop, fam.nfft
    return [0, 1, 2, 7, 8, 9, hop - 1, hop, hop + 1, nfft - 1, nfft, nfft + 1, 3 * nfft + 5]


def schedule(lengths, seed, choices):
    """Rounds of one chunk length per stream, each drawn on its own from ``choices``, until every stream is spent."""
    rng = np.random.default_rng(seed)
    pos = [0] * len(lengths)
    rounds = []
    while any(p < n for p, n in zip(pos, lengths)):
        cut = []
        for u, n in enumerate(lengths):
            c = min(int(rng.choice(choices)), n - pos[u])
            cut.append((pos[u], pos[u] + c))
            pos[u] += c
        rounds.append(cut)
    return rounds


def cat(rows, like):
    rows = [np.asarray(r) for r in rows]
    return np.concatenate(rows) if rows else like[:0]


def push_host(bank, xs, rounds):
    got = [[] for _ in xs]
    for cut in rounds:
        for u, r in enumerate(bank.push([x[a:b] for x, (a, b) in zip(xs, cut)])):
            got[u].append(r)
    return got


def push_dev(bank, xs, rounds):
    """Every round's chunks lie in ONE device tensor uploaded beforehand; all pushes are issued on a side stream with
    nothing between them, each into a tensor of the caller's, and only then is anything waited for or read."""
    import torch
    flats, offs = [], []
    for cut in rounds:
        chunks = [x[a:b] for x, (a, b) in zip(xs, cut)]
        offs.append(np.concatenate([[0], np.cumsum([len(c) for c in chunks])]).astype(np.uint64))
        flats.append(np.concatenate(chunks))
    starts = np.concatenate([[0], np.cumsum([len(f) for f in flats])])
    big = torch.from_numpy(np.concatenate(flats + [np.zeros(8, np.int16)])).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    outs = []
    with torch.cuda.stream(side):
        for k, off in enumerate(offs):
            flat = big[int(starts[k]):int(starts[k + 1])]
            nf = int(bank.num_frames(np.diff(off.astype(np.int64)))[-1])
            out = torch.empty((nf, bank._row()), device="cuda", dtype=torch.float32)
            res, fo = bank.push_packed(flat, off, out=out)
            assert res is out
            outs.append((out, fo))
    side.synchronize()
    got = [[] for _ in xs]
    for out, fo in outs:
        o = out.cpu().numpy()
        for u in range(len(xs)):
            got[u].append(o[int(fo[u]):int(fo[u + 1])])
    return got


def noise_then_const(fam, noise_frames, const_frames, pad, seed):
    """Noise, then constant -32768: from one frame past the step on every frame is the same row, so the variance of
    a window is exactly 0 once the noise has left it."""
    n = length(fam, noise_frames + const_frames, pad)
    x = np.full(n, -32768, np.int16)
    k = length(fam, noise_frames, "notebook")
    x[:k] = kf.signal("noise", k, seed, None)
    return x


class Model:
    """What N lagged sessions have returned and hold: the plan, in Python."""

    def __init__(self, fam, n, lag):
        self.nfft, self.hop, self.lag = fam.nfft, fam.hop, lag
        self.queued, self.held = [0] * n, [0] * n

    def push(self, lens):
        out = []
        for u, k in enumerate(lens):
            self.queued[u] += int(k)
            r = 0
            while self.queued[u] >= self.nfft:
                self.queued[u] -= self.hop
                self.held[u] += 1
                if self.held[u] > self.lag:
                    self.held[u] -= 1
                    r += 1
            out.append(r)
        return out
