"""Row-listed fp64 expand and gather, TEST INFRASTRUCTURE ONLY: tests/helpers/phaser_lr64.py restricted to a list of rows of
the full batch, the contract of mx_phaser_mod_expand_rows / mx_phaser_dmod_gather_rows.  Every array stays indexed by the
full-batch row; a listed row gets what the un-listed function gives it, the other rows of ``out`` are not touched."""
import numpy as np

from tests.helpers.phaser_lr64 import expand64, gather64


def expand64_rows(mod_lr, lead, rows, N, width, out):
    """mod_lr (B, n_mod), lead (B,), rows: a list of row indices in any order; writes the listed rows of ``out``
    (B, ceil(width / 4)) float64 and returns it."""
    mod_lr = np.asarray(mod_lr, np.float64)
    for b in rows:
        out[b] = expand64(mod_lr[b:b + 1], [lead[b]], N, width)[0]
    return out


def gather64_rows(dmod_g, lead, rows, N, n_mod, out):
    """dmod_g (B, n_groups), lead (B,), rows as above; writes the listed rows of ``out`` (B, n_mod) float64, returns it."""
    dmod_g = np.asarray(dmod_g, np.float64)
    for b in rows:
        out[b] = gather64(dmod_g[b:b + 1], [lead[b]], N, n_mod)[0]
    return out
