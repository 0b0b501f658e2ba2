"""The two forms of a segment pass's tile plan (mfcc_amd/csrc/seg_plan.hpp) through each of the
eight direct entries: normalize, PCEN, sliding normalization, deltas, VAD, selection, gate and gate windows.

Three equal segments of T + 1 rows -- T the pass's own tile rows, so every segment has a full tile and a one-row tile --
run through the uniform form, given once as a 3-D tensor without offsets and once as equal offsets, and through the
table form: the same three segments followed by one segment of a single row.  The results on the three common segments
must be bit-equal between the forms, the selection's offsets and packed rows and the gate's powers, masks and extracted
windows included.  No reference is needed: "a segment gives the same bits wherever it lies" is the kernels' contract.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WIDTHS = [13, 64]
SLIDE_WINDOW, DELTA_ORDER, DELTA_WINDOW = 50, 2, 2
GATE = dict(n_frames=5, stride=2)


def tile_rows(entry, width):
    """rows per tile of the entry's pass, as the kernel headers and DESIGN.md state them"""
    if entry == "normalize":
        return 8192 // width                                       # kernel_normalize.hpp: kTileFloats / W
    if entry == "pcen":
        return 128                                                 # kernel_pcen.hpp: kTile
    if entry == "sliding":
        return (256 // width) * max(32, min(256, SLIDE_WINDOW // 4))     # kernel_normalize_sliding.hpp: G runs
    if entry == "deltas":
        per = (4096 - 8) // width                                  # kernel_deltas.hpp: tile_rows(width, order, window)
        return (per - 2 * DELTA_WINDOW) // 3 if DELTA_ORDER == 1 else (per - 6 * DELTA_WINDOW) // 5
    if entry == "vad":
        return 4096                                                # kernel_vad.hpp: the mean's tile; the decision's is 1024
    if entry == "select":
        return min((4096 - 8) // width, 1024)                      # kernel_vad.hpp: select_tile_rows(width)
    raise KeyError(entry)


@pytest.fixture(scope="module")
def handle():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import mfcc_amd
    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13) as m:
        yield m


def forms(x3):
    """x3: (3, n, W) on the device.  (rows, frame_offsets) of the three forms; every tensor fresh"""
    import torch
    n, width = int(x3.shape[1]), int(x3.shape[2])
    flat = x3.reshape(3 * n, width)
    tail = torch.full((1, width), 0.5, device=x3.device, dtype=x3.dtype)
    return [(x3.clone(), None), (flat.clone(), np.arange(4) * n),
            (torch.cat([flat, tail]), np.array([0, n, 2 * n, 3 * n, 3 * n + 1]))]


def rows_of(entry, width, seed, lo=-4.0, hi=12.0):
    import torch
    n = tile_rows(entry, width) + 1
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.uniform(lo, hi, (3, n, width)).astype(np.float32)).cuda(), n


def common(t, n, per):
    """the entries of the three common segments (`per` of them per row), whatever the form's shape"""
    return t.reshape(-1)[:3 * n * per].cpu().numpy()


def assert_forms_equal(results):
    assert len(results) == 3
    for r in results[1:]:
        assert r.shape == results[0].shape and r.tobytes() == results[0].tobytes()


@pytest.mark.parametrize("width", WIDTHS)
def test_normalize(handle, width):
    x, n = rows_of("normalize", width, 1)
    assert_forms_equal([common(handle.normalize_rows(r, fo, mode="meanvar"), n, width) for r, fo in forms(x)])


@pytest.mark.parametrize("width", WIDTHS)
def test_pcen(handle, width):
    x, n = rows_of("pcen", width, 2)
    assert_forms_equal([common(handle.pcen_rows(r, fo), n, width) for r, fo in forms(x)])


@pytest.mark.parametrize("width", WIDTHS)
def test_sliding(handle, width):
    x, n = rows_of("sliding", width, 3)
    assert_forms_equal([common(handle.normalize_rows(r, fo, mode="meanvar", window=SLIDE_WINDOW, center=False), n, width)
                        for r, fo in forms(x)])


@pytest.mark.parametrize("width", WIDTHS)
def test_deltas(handle, width):
    x, n = rows_of("deltas", width, 4)
    assert_forms_equal([common(handle.deltas_rows(r, fo, order=DELTA_ORDER, window=DELTA_WINDOW), n, width * (1 + DELTA_ORDER))
                        for r, fo in forms(x)])


@pytest.mark.parametrize("width", WIDTHS)
def test_vad(handle, width):
    x, n = rows_of("vad", width, 5)
    got = [common(handle.vad_rows(r, fo, column=0, energy_threshold=1.0, energy_mean_scale=0.5, frames_context=2), n, 1)
           for r, fo in forms(x)]
    assert 0 < got[0].sum() < got[0].size                          # both answers occur
    assert_forms_equal(got)


@pytest.mark.parametrize("width", WIDTHS)
def test_select(handle, width):
    import torch
    x, n = rows_of("select", width, 6)
    voiced = torch.from_numpy((np.random.default_rng(7).random((3, n)) < 0.6).astype(np.uint8)).cuda()
    one = torch.ones(1, device="cuda", dtype=torch.uint8)
    masks = [voiced, voiced.reshape(-1).clone(), torch.cat([voiced.reshape(-1), one])]
    got = [handle.select_rows(r, v, fo) for (r, fo), v in zip(forms(x), masks)]
    offsets = [np.asarray(oo)[:4] for _, oo in got]
    kept = int(offsets[0][3])
    assert 0 < kept < 3 * n
    assert all(np.array_equal(o, offsets[0]) for o in offsets) and int(got[2][1][4]) == kept + 1
    assert_forms_equal([out[:kept].cpu().numpy() for out, _ in got])


def gate_rows(seed):
    """three segments of T + 1 windows (T = 1024 windows per tile of the power pass and of the extraction at n_cep 13,
    n_frames 5, stride 2: kernel_gate.hpp power_tile_wins, kSelTileWins)"""
    import torch
    n = 1024 * GATE["stride"] + GATE["n_frames"]
    assert (n - GATE["n_frames"]) // GATE["stride"] + 1 == 1025
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.integers(-3000, 3000, (3, n, 13)).astype(np.int16)).cuda(), n


def gate_forms(x3, n):
    """as forms(), for int16 rows; the odd segment has one row: no window"""
    import torch
    flat = x3.reshape(3 * n, 13)
    tail = torch.full((1, 13), 7, device=x3.device, dtype=x3.dtype)
    return [(x3, None), (flat, np.arange(4) * n), (torch.cat([flat, tail]), np.array([0, n, 2 * n, 3 * n, 3 * n + 1]))]


def test_gate(handle):
    x, n = gate_rows(8)
    got = [handle.gate_rows(r, fo, threshold=4000000, **GATE) for r, fo in gate_forms(x, n)]
    wo = [np.asarray(g[3])[:4] for g in got]
    assert list(wo[0]) == [0, 1025, 2050, 3075] and all(np.array_equal(w, wo[0]) for w in wo) and int(got[2][3][4]) == 3075
    gate = got[0][1].cpu().numpy()
    assert 0 < gate.sum() < gate.size                              # both answers occur
    for k in range(3):                                             # power, gate, gate_ref
        assert_forms_equal([g[k].cpu().numpy() for g in got])


def test_gate_windows(handle):
    import torch
    x, n = gate_rows(9)
    mask = torch.from_numpy((np.random.default_rng(10).random(3075) < 0.3).astype(np.uint8)).cuda()
    got = [handle.gate_windows(r, mask, fo, **GATE) for r, fo in gate_forms(x, n)]
    kept = int(mask.sum())
    assert 0 < kept < 3075
    offsets = [np.asarray(g[2])[:4] for g in got]
    assert int(offsets[0][3]) == kept and all(np.array_equal(o, offsets[0]) for o in offsets) and int(got[2][2][4]) == kept
    assert_forms_equal([g[0].cpu().numpy() for g in got])          # the windows
    assert_forms_equal([g[1].cpu().numpy() for g in got])          # their first rows: one flat numbering in all three forms
