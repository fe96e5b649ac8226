"""fp64 torch restatement of the pre-emphasis of mod_extraction/wright_code.py:47-73 and of the ESR taken after it
(losses.py:34-38), written from the formulas, not from the kernels:

  F       stage 1  f[n] = sum_k c[k] x[n-(K-1)+k], n = 0..T-1, x[<0] = 0
          stage 2  g[n] = 0.85 f[n] + f[n+1], n = 0..T-2                      (only with low_pass)
  F^T     the transpose of the two stages as explicit index sums
  value   w * mean_b ||F(y - y_hat)||^2 / (||F y||^2 + eps)
  grad    (2 w / B) F^T F (y_hat - y) / (||F y||^2 + eps)

Rows are the last dimension; everything is float64."""
import torch

LP = (0.85, 1.0)


def pre_emph64(x: torch.Tensor, taps, low_pass: bool) -> torch.Tensor:
    """F x: (..., T) -> (..., L), L = T or T - 1."""
    x = x.double()
    K, T = len(taps), x.size(-1)
    xp = torch.cat([x.new_zeros(x.shape[:-1] + (K - 1,)), x], dim=-1)
    f = sum(float(taps[k]) * xp[..., k:k + T] for k in range(K))
    if not low_pass:
        return f
    return LP[0] * f[..., :-1] + LP[1] * f[..., 1:]


def pre_emph_t64(v: torch.Tensor, taps, low_pass: bool, T: int) -> torch.Tensor:
    """F^T v: (..., L) -> (..., T)."""
    v = v.double()
    K = len(taps)
    if low_pass:
        assert v.size(-1) == T - 1
        h = v.new_zeros(v.shape[:-1] + (T,))
        h[..., :-1] += LP[0] * v                 # g[n] reads f[n] ...
        h[..., 1:] += LP[1] * v                  # ... and f[n+1]
    else:
        assert v.size(-1) == T
        h = v
    out = v.new_zeros(v.shape[:-1] + (T,))
    for k in range(K):                           # f[n] reads x[n-(K-1)+k]: x[j] collects c[k] h[j+(K-1)-k]
        s = K - 1 - k
        if s < T:
            out[..., :T - s] += float(taps[k]) * h[..., s:]
    return out


def esr_pre_value64(y_hat: torch.Tensor, y: torch.Tensor, taps, low_pass: bool, eps: float = 1e-8, w: float = 1.0):
    """(B, T) rows -> the weighted value (a 0-d float64 tensor)."""
    e = pre_emph64(y.double() - y_hat.double(), taps, low_pass)
    fy = pre_emph64(y, taps, low_pass)
    return w * ((e * e).sum(-1) / ((fy * fy).sum(-1) + eps)).mean()


def esr_pre_grad64(y_hat: torch.Tensor, y: torch.Tensor, taps, low_pass: bool, eps: float = 1e-8, w: float = 1.0):
    """(B, T) rows -> d value / d y_hat (B, T), by the explicit adjoint."""
    B, T = y_hat.shape
    r = pre_emph64(y_hat.double() - y.double(), taps, low_pass)
    fy = pre_emph64(y, taps, low_pass)
    den = (fy * fy).sum(-1, keepdim=True) + eps
    return (2.0 * w / B) * pre_emph_t64(r, taps, low_pass, T) / den
