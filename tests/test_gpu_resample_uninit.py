"""GPU: the resampler (K24) never depends on the contents of uninitialised device memory -- ``resample.resample_rows`` on both
routes (the tap table staged in LDS, and read through L2) under tests/helpers/poison_alloc.py with the 0 / 0.5 / NaN fills,
through the probe of tests/test_gpu_uninit_independence.py: every output bit-identical across the fills, no NaN under the NaN
fill, and the poisoned call sites named.  The wrapper takes the output from ``torch.empty``, and a fresh plan takes its tap
table from there too: every entry of the table and every output sample must be overwritten, and the zero padding at a row's
two ends must come from the kernel's bounds, not from memory beside the row."""
import numpy as np
import pytest

from tests.test_gpu_uninit_independence import _dv, _rng, run_patterns

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("sr_in, sr_out, route, n", [
    (48000, 44100, "lds", 4461),                # n_out = 4099: a full tile and three outputs of the next
    (44100, 32000, "l2", 5650),                 # n_out = 4100
    (44100, 32000, "l2", 3),                    # a row shorter than half a filter: every output is all edge
])
def test_resample_rows_on_each_route(dev, sr_in, sr_out, route, n):
    from mod_extraction_amd import resample
    assert resample.resample_plan(sr_in, sr_out).route == route
    wide = _dv(dev, _rng(n).standard_normal((3, n + 5)))
    x = wide[:, 2:2 + n]                                        # rows a stride apart, off the 16-byte boundary

    def case():
        plan = resample.resample_plan(sr_in, sr_out)            # a fresh plan: its table is allocated inside the case
        return {"y": resample.resample_rows(x, sr_in, sr_out, plan=plan), "taps": plan.taps(dev)}

    run_patterns(case, {"resample:resample_rows", "resample:taps"})
    y = resample.resample_rows(x, sr_in, sr_out)
    assert y.shape == (3, resample.resample_plan(sr_in, sr_out).out_length(n)) and bool(np.isfinite(y.cpu().numpy()).all())
