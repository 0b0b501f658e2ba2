"""The passes behind the float kernels -- VAD decision on the raw rows, PCEN, normalization (per segment or sliding),
deltas, voiced-row selection -- crossed with every route that runs them.

The reference is built WITHOUT the chain: a plain handle of the same parameters gives the raw rows (``process_batch`` on
device tensors), and the test composes the direct entries on them in the documented order: ``vad_rows``, ``pcen_rows``,
``normalize_rows`` (with or without a window), ``deltas_rows``, ``select_rows``.  Every route of a handle that has the
passes set must give those bits, per utterance:

1. ``process()`` per utterance on a device tensor (dense device route, one channel);
2. ``process()`` per utterance on a NumPy array (dense host route, one chunk);
3. ``process()`` on a stacked array of three equal-length utterances, device and host (several channels);
4. ``process_batch()`` on device tensors and on NumPy arrays (ragged, the table form of the tile plan);
5. ``process_packed()`` with three equal lengths (ragged, the equal-lengths fast path);
6. with ``MFCC_HIP_HOST_CHUNK_MB=1``: whole-channel chunks, frame-range chunks of one long channel, and a
   ``process_batch`` whose utterances cross a chunk edge -- against the same call on device tensors.

A ``vad="select"`` handle takes the ragged routes only; the dense ones must answer UNSUPPORTED.

The corpus is chosen so that segment edges and tile edges of every pass disagree: 300 frames with silent stretches
(three PCEN tiles, rows of -inf), 129 frames, 1 frame, no frame at all, 37 frames -- and 1300 frames, because the tile of
the per-segment normalization is 8192 / width rows (630 at width 13) and one segment has to span three of those too.
The tile sizes are read from the kernel headers.
"""
import itertools
import os
import re

import numpy as np
import pytest

import kernel_families as kf
from kernel_families import same

pytestmark = pytest.mark.gpu

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mfcc_amd", "csrc")
FAM = kf.FLOAT[0]                                                        # nfft 512, hop 170, 32 filters
FRAMES = [300, 129, 1, 0, 37, 1300]

OUTPUTS = {
    "cepstra": dict(nfft=512, nfilters=32, nceptrums=13),
    "logmel": dict(nfft=512, nfilters=32, nceptrums=13, output="logmel"),
    "logmel_pcen": dict(nfft=512, nfilters=32, nceptrums=13, output="logmel", pcen=True),
}
NORMS = {
    "raw": dict(),
    "meanvar": dict(normalize="meanvar"),
    "mean_w50": dict(normalize="mean", normalize_window=50, normalize_center=False, normalize_min_window=1),
}
VAD = dict(column=0, energy_threshold=0.0, energy_mean_scale=1.0, frames_context=2)
VAD_KW = dict(vad="select", **{"vad_" + k: v for k, v in VAD.items()})
CONFIGS = list(itertools.product(OUTPUTS, NORMS, (0, 2), (False, True)))
# routes 6: the two shapes of the staging -- every configuration with deltas, and one without
CHUNKED = [c for c in CONFIGS if c[2] == 2] + [("logmel_pcen", "meanvar", 0, False)]


def _id(c):
    return "%s-%s-d%d%s" % (c[0], c[1], c[2], "-vad" if c[3] else "")


def _header_int(header, name):
    src = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, header)).read())
    return int(re.search(r"^constexpr int %s = (\d+);" % name, src, flags=re.M).group(1))


@pytest.fixture(scope="module")
def mfcc_amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import mfcc_amd
    return mfcc_amd


@pytest.fixture(scope="module")
def corpus(wav_pcm):
    def n(frames):
        return FAM.hop * (frames - 1) + FAM.nfft if frames else 0        # an empty utterance

    xs = [kf.silent_stream(FAM, 300, 3), kf.signal("speech", n(129), 4, wav_pcm), kf.signal("noise", n(1), 5, wav_pcm),
          kf.signal("noise", n(0), 6, wav_pcm), kf.signal("silences", n(37), 7, wav_pcm),
          kf.signal("speech", n(1300), 8, wav_pcm)]
    return xs


def test_corpus_crosses_the_tiles_of_every_pass(mfcc_amd, corpus):
    with mfcc_amd.MFCC(**OUTPUTS["logmel"]) as m:
        assert [m.num_frames(len(x)) for x in corpus] == FRAMES
        assert np.isinf(m.process(corpus[0])).any()                      # rows of -inf
    pcen_tile = _header_int("kernel_pcen.hpp", "kTile")
    assert FRAMES[0] > 2 * pcen_tile and FRAMES[0] % pcen_tile           # three tiles, the last one short
    tile_floats = _header_int("kernel_normalize.hpp", "kTileFloats")
    for width in (13, 32):
        tile = tile_floats // width
        assert max(FRAMES) > 2 * tile and max(FRAMES) % tile, width


@pytest.fixture(scope="module")
def raw_rows(mfcc_amd, corpus):
    """Per output kind: the plain handle and its raw rows of every utterance, on the device.  Shared, never written."""
    import torch
    handles, rows = {}, {}
    for kind in ("cepstra", "logmel"):
        handles[kind] = mfcc_amd.MFCC(**OUTPUTS[kind])
        rows[kind] = handles[kind].process_batch([torch.from_numpy(x).cuda() for x in corpus])
        assert [len(r) for r in rows[kind]] == FRAMES
    handles["logmel_pcen"], rows["logmel_pcen"] = handles["logmel"], rows["logmel"]
    yield handles, rows
    for kind in ("cepstra", "logmel"):
        handles[kind].close()


def _compose(raw, rows, config):
    """The documented order on the raw rows of ONE utterance, by the direct entries of the plain handle ``raw``."""
    import torch
    output, norm, deltas, vad = config
    width = int(rows.shape[1])
    if len(rows) == 0:
        return torch.empty((0, width * (1 + deltas)), device=rows.device)
    rows = rows.clone()
    mask = raw.vad_rows(rows, **VAD) if vad else None
    if output == "logmel_pcen":
        raw.pcen_rows(rows)
    if norm == "meanvar":
        raw.normalize_rows(rows, mode="meanvar")
    elif norm == "mean_w50":
        rows = raw.normalize_rows(rows, mode="mean", window=50, min_window=1, center=False)
    if deltas:
        rows = raw.deltas_rows(rows, order=deltas, window=2)
    if vad:
        rows = raw.select_rows(rows, mask)[0]
    return rows


def _handle(mfcc_amd, config):
    output, norm, deltas, vad = config
    return mfcc_amd.MFCC(**OUTPUTS[output], **NORMS[norm], deltas=deltas, **(VAD_KW if vad else {}))


def _unsupported(mfcc_amd, call):
    from mfcc_amd import _lib as L
    with pytest.raises(mfcc_amd.MfccHipError) as e:
        call()
    return e.value.code == L.ERROR_UNSUPPORTED


@pytest.mark.parametrize("config", CONFIGS, ids=_id)
def test_every_route_gives_the_bits_of_the_composed_direct_entries(mfcc_amd, corpus, raw_rows, config):
    import torch
    handles, rows = raw_rows
    vad = config[3]
    want = [kf.as_np(_compose(handles[config[0]], r, config)) for r in rows[config[0]]]
    if vad:
        assert 0 < len(want[0]) < FRAMES[0] and len(want[3]) == 0
    dev = [torch.from_numpy(x).cuda() for x in corpus]
    bad = []

    def check(route, got, u):
        got = kf.as_np(got)
        if not same(got, want[u]):
            d = np.abs(got.astype(np.float64) - want[u]) if got.shape == want[u].shape else None
            bad.append((route, u, got.shape, want[u].shape, None if d is None or not d.size else float(np.nanmax(d))))

    with _handle(mfcc_amd, config) as m:
        for u in range(len(corpus)):
            check("1 process(device)", m.process(dev[u]), u)
            check("2 process(host)", m.process(corpus[u]), u)
        three = np.stack([corpus[0]] * 3)
        if vad:
            assert _unsupported(mfcc_amd, lambda: m.process(three))
            assert _unsupported(mfcc_amd, lambda: m.process(torch.from_numpy(three).cuda()))
        else:
            for route, got in (("3 stacked(host)", m.process(three)),
                               ("3 stacked(device)", m.process(torch.from_numpy(three).cuda()))):
                assert got.shape[0] == 3
                for c in range(3):
                    check(route, got[c], 0)
        for route, got in (("4 process_batch(device)", m.process_batch(dev)), ("4 process_batch(host)", m.process_batch(corpus))):
            assert len(got) == len(corpus)
            for u in range(len(corpus)):
                check(route, got[u], u)
        flat = torch.from_numpy(np.concatenate([corpus[0]] * 3)).cuda()
        out, fo = m.process_packed(flat, np.arange(4, dtype=np.uint64) * np.uint64(len(corpus[0])))
        for c in range(3):
            check("5 process_packed", out[int(fo[c]):int(fo[c + 1])], 0)
    assert not bad, bad


@pytest.mark.parametrize("config", CHUNKED, ids=_id)
def test_chunked_host_routes_give_the_bits_of_the_device_call(mfcc_amd, corpus, config, monkeypatch):
    """Routes 6.  The reference is the same call on device tensors, without the variable."""
    import torch
    vad = config[3]
    x = corpus[0]
    long = np.resize(x, 1_300_003)
    three = np.stack([long[:600_000], long[600_000:1_200_000], long[3:600_003]])
    batch = [long[:700_000], x, long[:600_001]]
    with _handle(mfcc_amd, config) as m:
        want_long = kf.as_np(m.process(torch.from_numpy(long).cuda()))
        want_batch = [kf.as_np(r) for r in m.process_batch([torch.from_numpy(b).cuda() for b in batch])]
        want_three = None if vad else kf.as_np(m.process(torch.from_numpy(three).cuda()))
        monkeypatch.setenv("MFCC_HIP_HOST_CHUNK_MB", "1")
        assert same(m.process(long), want_long), "frame-range chunks"
        if not vad:
            assert same(m.process(three), want_three), "whole-channel chunks"
        got = m.process_batch(batch)
        monkeypatch.delenv("MFCC_HIP_HOST_CHUNK_MB")
        for u in range(3):
            assert same(got[u], want_batch[u]), ("process_batch across a chunk edge", u)
        assert same(want_batch[1], m.process(x))
