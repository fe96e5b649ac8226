"""GPU: the track fit (K23) never depends on the contents of uninitialised device memory -- ``modulations.fit_lfo`` on its
``mx_track_fit`` route under tests/helpers/poison_alloc.py with the 0 / 0.5 / NaN fills, through the probe of
tests/test_gpu_uninit_independence.py: every output bit-identical across the fills, no NaN under the NaN fill, and the poisoned
call site named.  The wrapper takes the workspace (the tiles' partial argmins, the centred fp64 row, the row's mean and Syy,
each shape's refined result), the six outputs and the per-shape table from ``torch.empty``.  A constant row and a mask that
leaves shapes out are among the cases: their workspace words are written by nobody, and must be read by nobody."""
import numpy as np
import pytest
import torch

from tests.helpers import lfo_fit64 as h
from tests.test_gpu_uninit_independence import _dv, _rng, run_patterns

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n, window, shapes", [
    (345, (0.25, 80.0), ("cos", "rect_cos", "inv_rect_cos", "tri", "saw", "rsaw")),      # K = 639: 80 candidate tiles a shape
    (4097, (0.9, 1.5), ("tri", "sqr")),                                                    # three row tiles; five shapes masked out
])
def test_fit_lfo_on_the_track_route(dev, n, window, shapes):
    from mod_extraction_amd import modulations as M
    assert M.fit_plan(n, 172.5, window)[0] == "track_fit"
    r = _rng(n)
    y = np.stack([h.make_row(n, 172.5, "tri", 1.2, 2.0, noise=0.02, rng=r), np.full(n, 0.3, dtype=np.float32),
                  h.make_row(n, 172.5, "cos", 1.1, 0.4)])
    yd = _dv(dev, y)

    def case():
        return M.fit_lfo(yd, 172.5, window, shapes=shapes, per_shape=True)._asdict()

    run_patterns(case, {"modulations:fit_lfo"})
    fit = M.fit_lfo(yd, 172.5, window, shapes=shapes, per_shape=True)
    assert fit.shape.tolist()[0] == 3 and fit.amp.tolist()[1] == 0.0 and fit.resid.tolist()[1] == 0.0
    assert bool(torch.isinf(fit.per_shape_resid[:, [i for i in range(7) if h.SHAPES[i] not in shapes]]).all())
