"""Golden vectors for the pre-emphasis of mod_extraction/wright_code.py -> wright_pre_emph.npz: seeded time-major
(T, B, 1) inputs with the outputs of the REAL ``WrightPreEmph`` on them, and the values of ``WrightESRLoss`` /
``WrightDCLoss`` (wright_code.py:15-41) and of ``ESRLoss`` (losses.py:14-38) on the filtered pairs.  Taps [-0.95, 1]
(Wright & Valimaki), [1.0] and [0.2, -0.9, 1.0], each with low_pass off and on; (T, B) in {(2, 1), (257, 3), (4099, 2)}.
The reference's losses.py imports auraloss and torchaudio at module level, which ESRLoss never touches: empty
placeholder modules stand in for them, as in make_golden_nn.py.  Row 1 of the two larger shapes has a SILENT target and a prediction at 1e-6, so that ESRLoss's eps 1e-8 decides that
clip's ratio while the value stays of order 1.  Only the vectors are committed.

    cd tests/golden && PYTHONDONTWRITEBYTECODE=1 python make_golden_wright.py <path of the reference checkout>
"""
import os
import sys
import types

import numpy as np
import torch as tr

HERE = os.path.dirname(os.path.abspath(__file__))
TAPS = [[-0.95, 1.0], [1.0], [0.2, -0.9, 1.0]]
SHAPES = [(2, 1), (257, 3), (4099, 2)]          # (T, B)


def main(ref: str) -> None:
    sys.path.insert(0, ref)
    sys.dont_write_bytecode = True
    for name, attr in (("auraloss", None), ("auraloss.freq", None), ("torchaudio", None),
                       ("torchaudio.transforms", "MelSpectrogram")):
        if name not in sys.modules:                     # never called: the fixture must not depend on them
            sys.modules[name] = types.ModuleType(name)
            if attr:
                setattr(sys.modules[name], attr, None)
    from mod_extraction import losses as rlosses, wright_code as rw
    out = {f"taps_{i}": np.asarray(t, np.float32) for i, t in enumerate(TAPS)}
    tr.manual_seed(1502)
    for T, B in SHAPES:
        n = tr.arange(T, dtype=tr.float32).view(T, 1, 1) / 44100.0
        tgt = 0.4 * tr.sin(2 * np.pi * 220.0 * n + tr.rand(1, B, 1) * 6.0) + 0.3 * (tr.rand(T, B, 1) - 0.5) + 0.05
        pred = 0.8 * tgt + 0.05 * (tr.rand(T, B, 1) - 0.5) - 0.01
        if B > 1:
            tgt[:, 1] = 0.0
            pred[:, 1] = 1e-6 * (tr.rand(T, 1) * 2 - 1)
        out[f"out_T{T}"], out[f"tgt_T{T}"] = pred.numpy().copy(), tgt.numpy().copy()
        for i, taps in enumerate(TAPS):
            for lp in (0, 1):
                key = f"T{T}_k{i}_lp{lp}"
                with tr.no_grad():
                    f_out, f_tgt = rw.WrightPreEmph(taps, low_pass=bool(lp))(pred, tgt)
                    out["f_out_" + key], out["f_tgt_" + key] = f_out.numpy().copy(), f_tgt.numpy().copy()
                    out["wesr_" + key] = rw.WrightESRLoss()(f_out, f_tgt).numpy()
                    out["wdc_" + key] = rw.WrightDCLoss()(f_out, f_tgt).numpy()
                    # ESRLoss takes (B, 1, L)
                    out["esr_" + key] = rlosses.ESRLoss()(f_out.permute(1, 2, 0), f_tgt.permute(1, 2, 0)).numpy()
    path = os.path.join(HERE, "wright_pre_emph.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    print({k: (v.shape if v.ndim else float(v)) for k, v in out.items() if not k.startswith("f_")})


if __name__ == "__main__":
    main(sys.argv[1])
