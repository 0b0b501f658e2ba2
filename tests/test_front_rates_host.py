"""Fronted handles at the sample rates that change a kernel's form, on the CPU: what tests/test_gpu_front_rates.py relies
on, proven without a GPU.

* not blind: for every (case, front) of ``front_rate_cases.cases()`` x ``FRONTS`` -- and for the ``stream`` / ``halo=1``
  framing of ``stream_cases()`` -- the bound of the three bounded channels gives up nothing but frames x empty bands;
* the section-2 bound of the DC bands (``front_rate_cases.dc_reference_and_bound``) against the section-1 bound, element
  by element, see below;
* both exactness claims of the pre-emphasis at their loud end: ``preemph8``'s biased dot product and the generic kernels'
  ``fmaf``, restated in NumPy, on the four corner pairs and a million random full-scale pairs, with a pair just beyond
  each claim that is NOT exact, so that the check is known to see the edge;
* the loud stimuli reach ``max |e| = den 32768 + num 32767``;
* the four-wave table builders at 24 / 64 / 192 kHz, 32 and 16 filters, every front (tests/front_tables_driver.cpp).

Section 2 against section 1 (measured here, printed by the test).  The check was meant to be at least 8 times tighter
than section 1 on ``const_min`` and ``dc_dither``.  It cannot be on ``dc_dither`` or on any input that puts its energy
into bin 0: the fp32 FFT allowance of section 1 is ``2 |X0| e`` with ``e = u rms(X) log2(nfft)``, and where ``rms(X)
<= |X0|`` that is already below one fp32 rounding of ``P0``.  Measured: ratio section 1 / section 2 between 0.994 and
1.02 on ``dc_dither`` at every case and front.  What section 2 does gain:

* ``const_min`` at ``L = nfft`` (log-mel handles): every band away from DC is float64 roundoff of an exact zero, so the
  section-1 bound gives the whole row up (+inf) in every frame behind the first; section 2 pins the DC bands there to
  1.1e-5 log2 units.
* ``dc_under_tone`` (a full-scale period-8 square wave on a constant of 150): bin 0 lies far below the frame's rms.  On
  the log-mel handles, at the fronts with pre-emphasis and behind frame 0, section 1 is 19 to 2600 times looser (or
  +inf); the smallest factor is 19, on mfcc_fused512_h160_kernel under (povey, 32/33).

These are the (case, front, channel) triples ``gains()`` names, and the test asserts the factor of 8 on every element
of them.  The other triples run on the GPU all the same and are held to the section-2 bound; there it duplicates
section 1 (no factor is claimed).  A handle that returns only cepstra (mfcc_fused512_kernel) is read through the inverse
DCT, which brings every band's rounding back into the DC band, and only in frames where every band is determined: its
ratios stay below 8 in all but single frames and no factor is claimed either.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import front_rate_cases as fc
import front_ref as fr
import logmel_bound as lb
import test_rate_map_host as rmap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mfcc_amd", "csrc")
CASES = fc.cases()


# ---------------------------------------------------------------------------------------------------- 1. not blind
def test_the_case_list_holds_every_form():
    by_form = {}
    for c in CASES:
        kw = c.kw
        rate, n_mel = int(kw["samplerate"]), kw["nfilters"]
        if kw["nfft"] == 512 and kw.get("mel") != "htk":
            form = ("sparse" if rate in rmap.SPARSE_512 and n_mel == 32 else "dense",
                    rate in rmap.DC_EXACT[n_mel], bool(rmap.empty_bands(512, n_mel, rate)))
            by_form.setdefault((c.fused, form), []).append(c.id)
            assert (len(c.dc_bands()) > 0) == (rate in rmap.DC_EXACT[n_mel]), c.id
            assert lb.empty_bands(c.filters()).sum() == len(rmap.empty_bands(512, n_mel, rate)), c.id
        elif kw["nfft"] == 1024:
            assert (len(c.dc_bands()) > 0) == (rate in rmap.DC_1024), c.id
            assert lb.empty_bands(c.filters()).sum() == len(rmap.empty_bands(1024, 40, rate)), c.id
    for kernel in (fc.W4, fc.H160):
        forms = {f for k, f in by_form if k == kernel}
        assert ("sparse", False, False) in forms and ("dense", True, False) in forms and ("dense", True, True) in forms, forms
    assert ("dense", False, False) in {f for k, f in by_form if k == fc.W4}
    assert {c.fused for c in CASES} == {fc.W4, fc.H160, fc.H160MB, fc.GENERIC}
    assert {c.fused for c in fc.stream_cases()} == {fc.W4, fc.H160, fc.H160MB, fc.GENERIC}
    assert len(CASES) == 37


@pytest.mark.parametrize("front", fc.FRONTS, ids=fr.front_id)
def test_the_gpu_cases_are_not_blind(wav_pcm, front):
    worst = 0.0
    for case in CASES:
        fc.assert_not_blind(case, front, wav_pcm)
        for c in range(len(fc.BOUNDED)):
            b = fc.reference(case, front, wav_pcm, c)[1]
            worst = max(worst, float(b[np.isfinite(b)].max(initial=0.0)))
    for case in fc.stream_cases():
        fc.assert_not_blind(case, front, wav_pcm, "stream", 1)
    print("%s: largest finite bound of a bounded channel %.3g" % (fr.front_id(front), worst))
    assert worst < 0.25                      # 0.244: the DC band of ``uniform`` under (97, 100) at 192 kHz, 16 filters


# ---------------------------------------------------------------------------------------------------- 2. the DC bin
def _gain(b1, b2):
    """Per element: section 1 / section 2 where both are finite, +inf where only section 2 is, 0 where section 2 is not."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(np.isfinite(b2), np.where(np.isfinite(b1), b1 / b2, np.inf), 0.0)


def gains(case, front, kind):
    """Whether section 2 claims the factor ``DC_RATIO`` on this triple (behind frame 0): the module docstring."""
    if not case.logmel:
        return False
    if kind == "const_min":
        return case.frame_len == case.kw["nfft"]
    return kind == "dc_under_tone" and front[2][0] > 0


def test_the_dc_bound_is_a_check_of_its_own(wav_pcm):
    cases = fc.dc_cases()
    assert {c.kernel(fc.R) for c in cases} == {fc.W4, fc.H160, fc.GENERIC} and len(cases) == 10
    claimed, smallest = 0, np.inf
    for case in cases:
        x = fc.dc_channels(case.n_samples)
        for front in fc.FRONTS:
            for k, kind in enumerate(fc.DC_KINDS):
                if kind == "const_min" and front not in fc.DC_FRONTS:
                    continue
                ref, b2, b1 = fc.dc_reference_and_bound(case, front, x[k])
                assert ref.shape == b2.shape == b1.shape == (fc.NFR, len(case.dc_bands()))
                g = _gain(b1, b2)
                fin = np.isfinite(b2)
                print("%-42s %-22s %-13s section 2 <= %.3g (finite in %3.0f %%), section 1 / section 2 >= %.3g, >= 8 in %3.0f %%"
                      % (case.id, fr.front_id(front), kind, b2[fin].max(initial=0.0), 100 * fin.mean(), g[fin].min(initial=np.inf),
                         100 * (g >= fc.DC_RATIO).mean()))
                if case.logmel:                   # a log-mel handle: section 2 pins every DC band of every frame
                    assert fin.all() and np.isfinite(ref).all(), (case.id, front, kind)
                if gains(case, front, kind):
                    assert (g[1:] >= fc.DC_RATIO).all(), (case.id, front, kind, float(g[1:].min()))
                    claimed += 1
                    smallest = min(smallest, float(g[1:].min()))
    print("factor claimed on %d triples, smallest %.3g" % (claimed, smallest))
    assert claimed == 7 * 3 + 4 * 2 and smallest >= fc.DC_RATIO     # the tone on 7 log-mel handles, const_min at L = nfft on 4


def test_a_constant_under_the_rectangular_window_has_no_leakage():
    """L = nfft, periodic rectangular: behind frame 0 the reference's other bins are exactly 0 -- the sharpest case."""
    case = [c for c in fc.dc_cases() if c.id == "512/170 32 filters logmel at 64000"][0]
    x = fc.dc_channels(case.n_samples)[0]
    p = fr.power_reference(x, fc.R, 512, 170, 512, power_scale=512.0)
    assert (p[1:, 1:] == 0).all() and (p[1:, 0] == (32768.0 * 512 / 64 / 512) ** 2).all() and (p[0, 1:] > 0).all()


# ---------------------------------------------------------------------------------------------------- 4. exactness
CORNERS = [(a, b) for a in (32767, -32768) for b in (32767, -32768)]


def _pairs():
    rng = np.random.default_rng(8)
    x0 = np.concatenate([[a for a, _ in CORNERS], rng.integers(-32768, 32768, 1_000_000)])
    x1 = np.concatenate([[b for _, b in CORNERS], rng.integers(-32768, 32768, 1_000_000)])
    # full scale: half of the random pairs at the rails
    x0[4::2] = np.where(x0[4::2] < 0, -32768, 32767)
    x1[4::4] = np.where(x1[4::4] < 0, -32768, 32767)
    return x0.astype(np.int64), x1.astype(np.int64)


def test_the_biased_dot_product_is_exact_up_to_the_fused_limit():
    """``preemph8``: exact for every ``num + den <= 127`` (the limit the host builds the fused tables for).  The bias
    holds while ``12582912 + e`` stays in ``[2^23, 2^24)``, i.e. ``-2^22 <= e < 2^22``; ``max |e| = den 32768 + num 32767
    = (num + den) 2^15 - num``, so ``num + den = 128`` -- (63, 65) -- is still exact on all four corners (``|e| <= 2^22 -
    63``: no int16 pair reaches 2^22 there), and the first pair that is not is (64, 65), on the two corners of
    opposite signs: ``e = 4227007 >= 2^22`` and ``e = -4227008 < -2^22``."""
    x0, x1 = _pairs()
    c0, c1 = x0[:4], x1[:4]
    pairs = [(num, den) for den in range(1, 128) for num in range(0, min(den, 127 - den) + 1)]
    assert len(pairs) == 4159 and (64, 64) not in pairs and (63, 64) in pairs and (1, 126) in pairs and (31, 32) in pairs
    for num, den in pairs:                        # every pair the fused kernels serve, on the four corners
        assert np.array_equal(fc.preemph8_restated(c0, c1, num, den).astype(np.int64), den * c0 - num * c1), (num, den)
    # the million full-scale pairs: every pair at the limit num + den = 127, and the default
    for num, den in [(127 - den, den) for den in range(64, 128)] + [(31, 32)]:
        e = den * x0 - num * x1
        assert np.abs(e).max() < 2 ** 22
        assert np.array_equal(fc.preemph8_restated(x0, x1, num, den).astype(np.int64), e), (num, den)
    # num + den = 128 is beyond what the host builds, but still inside the binade
    assert np.array_equal(fc.preemph8_restated(c0, c1, 63, 65).astype(np.int64), 65 * c0 - 63 * c1)
    assert np.abs(65 * c0 - 63 * c1).max() == 2 ** 22 - 63
    # ... and the edge is seen: (64, 65) leaves the binade on the two corners of opposite signs
    e = 65 * c0 - 64 * c1
    got = fc.preemph8_restated(c0, c1, 64, 65).astype(np.float64)
    wrong = got != e
    assert wrong.tolist() == [a * b < 0 for a, b in CORNERS] and e[wrong].tolist() == [4227007, -4227008]
    assert e[wrong][0] >= 2 ** 22 and e[wrong][1] < -2 ** 22
    assert got[wrong][1] == 2.0 ** 23 - (4227008 - 2 ** 22) / 2.0 - 12582912.0      # the bits read in the binade below


def test_the_generic_fmaf_is_exact_up_to_its_limit():
    """``fmaf(-num, x[i-1], den x[i])``: an exact integer for every ``num + den <= 255`` (``|e| < 2^23``), (127, 128)
    included; (256, 257) reaches an odd ``|e| > 2^24`` on a corner and is not."""
    x0, x1 = _pairs()
    for num, den in [(127, 128), (97, 100), (0, 255), (1, 254), (120, 135), (31, 32), (63, 64), (0, 1), (1, 1)] + \
                    [(255 - d, d) for d in range(128, 256, 9)]:
        assert num + den <= 255 and num <= den
        e = den * x0 - num * x1
        assert np.abs(e).max() < 2 ** 23
        assert np.array_equal(fc.fmaf_restated(x0, x1, num, den).astype(np.int64), e), (num, den)
    c0, c1 = x0[:4], x1[:4]
    e = 257 * c0 - 256 * c1
    assert (fc.fmaf_restated(c0, c1, 256, 257).astype(np.int64) != e).any() and np.abs(e).max() > 2 ** 24


def test_the_loud_stimuli_reach_the_extreme(wav_pcm):
    n = 170 * (fc.LOUD_FRAMES - 1) + 512
    x = fc.loud_channels(n, wav_pcm)
    for front in (fc.R, fc.QUIET, fr.DEFAULT, fc.LOUD_GENERIC, fc.G):
        num, den = front[2]
        top = den * 32768 + num * 32767
        for c, kind in enumerate(fc.LOUD_KINDS):
            m = fc.max_abs_e(x[c], num, den)
            assert (m == top) == (kind != "speech") and m <= top, (front, kind, m, top)
        assert top < (2 ** 22 if fr.fused_pair(front) else 2 ** 23)
    assert fc.max_abs_e(x[0], 63, 64) < 0.5 * (64 * 32768 + 63 * 32767)       # speech is the quiet neighbour


# ---------------------------------------------------------------------------------------------------- 5. host driver
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = tmp_path_factory.mktemp("front_rate_tables") / "driver"
    subprocess.run([hipcc, "--cuda-host-only", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", "-Werror", "-I", CSRC,
                    "-o", str(exe), os.path.join(ROOT, "tests", "front_tables_driver.cpp")], check=True)
    return str(exe)


def test_dense_tables_at_other_rates_carry_the_front_and_the_default_bank(driver):
    """rate x filter count x front x frame length: ``needs_dc_exact`` is ``rmap.DC_EXACT``, the ``win_dc`` rows are ``w /
    den`` in double (behind ``set_window`` at 400 too), every mel operand is the default front's."""
    lines, keys = [], []
    for rate in (24000, 64000, 192000):
        for n_mel in (32, 16):
            for front in fr.FRONTS + [fc.QUIET]:
                for L in (512, 400):
                    kind, periodic, (num, den) = front
                    lines.append("%d %d %d %d %d %d %d" % (fr.KINDS.index(kind), int(not periodic), num, den, L, rate, n_mel))
                    keys.append((rate, n_mel, front, L))
    out = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(lines)
    counts = set()
    for (rate, n_mel, front, L), line in zip(keys, out):
        if not fr.fused_pair(front):              # (97, 100): a pair the fused kernels do not serve is refused here too
            assert line == "FAIL dense builder refused", (rate, n_mel, front, L, line)
            continue
        tag, dc, checked = line.split()
        assert tag == "ok" and int(dc) == int(rate in rmap.DC_EXACT[n_mel]), (rate, n_mel, front, L, line)
        counts.add(int(checked))
    assert len(counts) == 1 and min(counts) > 16 * 32 + 4 * 32 * 64, counts      # win_dc and every operand, the same for all
