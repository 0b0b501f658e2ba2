"""A fixed slice of the randomized soak (tests/soak_gpu.py) in front of the driver: 300 seeded cases -- ragged
batches, the fixed-point kernel bit for bit on every signal kind, both float kernels against the per-coefficient
error bound of the float64 oracle (oracle/error_bound.py) at random shapes, alignments, sample rates and filter counts.  `python tests/soak_gpu.py --case SEED`
replays a failing case."""
import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _soak():
    spec = importlib.util.spec_from_file_location("soak_gpu", os.path.join(HERE, "soak_gpu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("seed0", [31, 32, 33])
def test_soak_slice(seed0):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    soak = _soak()
    fails = []
    for k in range(100):
        seed = seed0 * 10_000_000 + k
        fails += ["[--case %d] %s" % (seed, f) for f in soak.one_case(seed)]
    assert not fails, fails
    # nothing is set aside: the DC / square / sine channels were held to the bound like the noise-like ones
    counted = {kind for _, kind in soak.WORST}
    assert {"dc", "square", "sine", "gauss"} <= counted, soak.summary()
    assert max(soak.WORST.values()) <= 1.0, soak.summary()
    print(soak.summary())
