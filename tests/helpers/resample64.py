"""numpy fp64 restatement of the rational resampler (K24; mod_extraction_amd/csrc/resample_abi.h has the definition): the plan,
the prototype, the tap table and the rows.  Written from the header's text with numpy only; ``rows`` takes an optional tap
table, so each stage of the kernels can be checked on the inputs the next stage really gets."""
import math
from typing import NamedTuple, Optional

import numpy as np

OUT_TILE = 4096
LDS_TABLE_BYTES = 160 * 1024
ROUTE_LDS, ROUTE_L2 = 0, 1
MAX_FACTOR, MAX_TAPS, MAX_TABLE, MAX_SPAN = 4096, 4095, 1 << 24, 1 << 62


class Plan(NamedTuple):
    up: int
    down: int
    half: int
    taps_per_phase: int
    c: float
    route: int

    def out_length(self, n_in: int) -> int:
        return -((-n_in * self.up) // self.down)


def plan(sr_in: int, sr_out: int, zeros: int = 48, rolloff: float = 0.95, beta: float = 16.0) -> Plan:
    g = math.gcd(sr_in, sr_out)
    up, down = sr_out // g, sr_in // g
    c = rolloff * (up / down if up < down else 1.0)
    half = int(math.ceil(zeros / c))
    T = 2 * half + 1
    return Plan(up, down, half, T, c, ROUTE_LDS if 4 * up * T <= LDS_TABLE_BYTES else ROUTE_L2)


def i0(x: float) -> float:
    """The power series in ascending j, until a term falls below 2^-60 of the sum."""
    q = 0.25 * x * x
    term = total = 1.0
    for j in range(1, 1000):
        term = term * q / (float(j) * float(j))
        total += term
        if term < total * 2.0 ** -60:
            break
    return total


def prototype(tau: np.ndarray, pl: Plan, beta: float = 16.0) -> np.ndarray:
    """h(tau), tau in input samples (fp64 array)."""
    tau = np.asarray(tau, dtype=np.float64)
    inside = np.abs(tau) <= pl.half
    r = np.where(inside, tau / pl.half, 0.0)
    arg = beta * np.sqrt(np.maximum(0.0, 1.0 - r * r))
    w = np.array([i0(float(a)) for a in arg.ravel()]).reshape(arg.shape) / i0(beta)
    return np.where(inside, pl.c * np.sinc(pl.c * tau) * w, 0.0)


def taps(pl: Plan, beta: float = 16.0) -> np.ndarray:
    """(up, T) fp64: h(((half - k) up + p) / up), not yet rounded to fp32."""
    p = np.arange(pl.up, dtype=np.int64)[:, None]
    k = np.arange(pl.taps_per_phase, dtype=np.int64)[None, :]
    num = (pl.half - k) * pl.up + p
    h = prototype(num.astype(np.float64) / float(pl.up), pl, beta)
    return np.where(np.abs(num) <= pl.half * pl.up, h, 0.0)


def index(m, pl: Plan):
    """(i0, p) = divmod(m down, up), exact (Python ints or int64 arrays)."""
    return np.divmod(np.asarray(m, dtype=np.int64) * pl.down, pl.up)


def rows(x: np.ndarray, pl: Plan, table: Optional[np.ndarray] = None, beta: float = 16.0, with_bound: bool = False):
    """(B, n_out) fp64 from x (B, n_in) or (n_in,): sum_k table[p][k] x[i0 - half + k], x zero outside the row.  ``table``: an
    (up, T) tap table (the kernel's fp32 one, say); by default the fp32 rounding of ``taps``.  ``with_bound`` adds sum |terms|."""
    x = np.asarray(x, dtype=np.float64)
    one = x.ndim == 1
    x = np.atleast_2d(x)
    table = (taps(pl, beta).astype(np.float32) if table is None else np.asarray(table)).astype(np.float64)
    assert table.shape == (pl.up, pl.taps_per_phase)
    B, n_in = x.shape
    n_out = pl.out_length(n_in)
    xp = np.zeros((B, n_in + 2 * pl.half + pl.taps_per_phase), dtype=np.float64)
    xp[:, pl.half:pl.half + n_in] = x
    y = np.zeros((B, n_out), dtype=np.float64)
    a = np.zeros((B, n_out), dtype=np.float64)
    i0_, p = index(np.arange(n_out), pl)
    for k in range(pl.taps_per_phase):                           # ascending k, as the kernel sums
        t = table[p, k][None, :] * xp[:, i0_ + k]
        y += t
        a += np.abs(t)
    if one:
        y, a = y[0], a[0]
    return (y, a) if with_bound else y
