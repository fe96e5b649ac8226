"""CPU: the surface of the FIR match (K21) -- its six declarations in include/modex_hip.h against ``_hip.SIGNATURES``, the
limits of the six entry points (checked before any launch, so without a device), the ``ValueError``s of the wrappers in
``mod_extraction_amd.fir_match`` and of the step's constructor, and the shipped config.  No device work."""
import ctypes
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"mx_fir_match_partials": 10, "mx_fir_match_solve": 12, "mx_fir_match_apply": 10, "mx_fir_match_bwd_partials": 10,
         "mx_fir_match_bwd_solve": 12, "mx_fir_match_bwd_apply": 16}
ARG, UNSUPPORTED = -1, -2


def test_header_table_and_symbols():
    """Exactly the six ``mx_fir_`` names, declared in include/modex_hip.h -- the one header: ``include/`` holds no other, and
    csrc/common.h includes no other -- and read here with a regex of this test's own; each is exported; argument counts and
    the bound argtypes are those of ``_hip.SIGNATURES``, which is what the parser makes of that text (ABI 21)."""
    from mod_extraction_amd import _hip, build, fir_match
    lib = ctypes.CDLL(build.build(verbose=False))
    assert [f for f in os.listdir(os.path.join(ROOT, "include")) if f.endswith(".h")] == ["modex_hip.h"]
    raw = open(os.path.join(ROOT, "include", "modex_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    counts = {n: len(a.split(",")) for n, a in re.findall(r"\bint\s+(mx_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)
              if n.startswith("mx_fir_")}
    assert counts == NAMES and list(counts) == [n for n in _hip.SIGNATURES if n.startswith("mx_fir_")]
    assert {k: len(_hip.SIGNATURES[k]) for k in NAMES} == NAMES
    assert all(n.startswith("mx_fir_") and not n.startswith(("mx_gain_match_", "mx_pair_")) for n in NAMES)
    assert _hip.SIGNATURES == _hip.parse_signatures(raw) and _hip.ABI_VERSION == 21
    P, I64, I32, F64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_double
    assert _hip.SIGNATURES["mx_fir_match_solve"] == [P, I64, I64, I64, I64, F64, F64, F64, P, P, P, P]
    assert _hip.SIGNATURES["mx_fir_match_bwd_apply"] == [P, I64, P, I64, P, I64, P, P, P, I64, I64, I64, I64, P, I64, P]
    assert int(re.search(r"^#define MX_FIR_CHUNK (\d+)$", raw, flags=re.M).group(1)) == fir_match.CHUNK
    assert int(re.search(r"^#define MX_FIR_MAX_TAPS (\d+)$", raw, flags=re.M).group(1)) == fir_match.MAX_TAPS == 32
    common = open(os.path.join(ROOT, "mod_extraction_amd", "csrc", "common.h")).read()
    assert re.findall(r'#include\s+"(modex_hip\w*\.h)"', common) == ["modex_hip.h"]
    zeros = {P: None, I64: 0, I32: 0, F64: 0.0}
    loaded = _hip.load()
    for name in NAMES:
        assert hasattr(lib, name)
        fn = getattr(loaded, name)
        assert fn.argtypes == _hip.SIGNATURES[name] and fn.restype is ctypes.c_int        # load() binds the one table
        assert fn(*[zeros[t] for t in fn.argtypes]) in (ARG, UNSUPPORTED)


def p(v):
    return None if v is None else ctypes.c_void_p(v)


A0, B0, C0, D0 = 1 << 20, 2 << 20, 3 << 20, 4 << 20                          # four row blocks that are far apart
W0, W1, W2, W3, W4, W5 = (5 << 20, 6 << 20, 7 << 20, 8 << 20, 9 << 20, 10 << 20)     # and six small arrays


def lib():
    from mod_extraction_amd import _hip
    return _hip.load()


def partials(y_hat=A0, y=B0, B=4, N=1000, K=9, c=4, s1=None, s2=None, ws=W0):
    return lib().mx_fir_match_partials(p(y_hat), N if s1 is None else s1, p(y), N if s2 is None else s2, B, N, K, c, p(ws), None)


def bwd_partials(dz=A0, y_hat=B0, B=4, N=1000, K=9, c=4, s1=None, s2=None, ws=W0):
    return lib().mx_fir_match_bwd_partials(p(dz), N if s1 is None else s1, p(y_hat), N if s2 is None else s2, B, N, K, c, p(ws), None)


def solve(ws=W0, B=4, nc=1, K=9, c=4, ridge=1e-6, eps=1e-8, max_gain=20.0, outs=(W1, W2, W3)):
    return lib().mx_fir_match_solve(p(ws), B, nc, K, c, ridge, eps, max_gain, *[p(o) for o in outs], None)


def apply(x=A0, taps=W1, B=4, N=1000, K=9, c=4, z=B0, s1=None, sz=None):
    return lib().mx_fir_match_apply(p(x), N if s1 is None else s1, p(taps), B, N, K, c, p(z), N if sz is None else sz, None)


def bwd_solve(ins=(W0, W2, W1, W3), B=4, nc=1, K=9, ridge=1e-6, eps=1e-8, outs=(W4, W5)):
    return lib().mx_fir_match_bwd_solve(*[p(i) for i in ins], B, nc, K, ridge, eps, *[p(o) for o in outs], None)


def bwd_apply(dz=A0, y=B0, y_hat=C0, small=(W1, W4, W5), B=4, N=1000, K=9, c=4, out=D0, s=(None,) * 4):
    st = [N if v is None else v for v in s]
    return lib().mx_fir_match_bwd_apply(p(dz), st[0], p(y), st[1], p(y_hat), st[2], *[p(i) for i in small], B, N, K, c, p(out),
                                        st[3], None)


BAD_EPS = (0.0, -1e-8, math.inf, math.nan)
BAD_RIDGE = (-1e-9, math.inf, math.nan)
BAD_MAX_GAIN = (0.5, 0.0, -1.0, math.inf, math.nan)


def test_limits_are_checked_before_any_launch():
    """Every case is refused on pointers that are never read (a case that would launch is not tried here)."""
    for fn, first, second in ((partials, "y_hat", "y"), (bwd_partials, "dz", "y_hat")):
        assert fn(**{first: None}) == ARG and fn(**{second: None}) == ARG and fn(ws=None) == ARG
        assert fn(B=0) == ARG and fn(B=-2) == ARG and fn(N=0) == ARG and fn(N=-5) == ARG
        assert fn(s1=999) == ARG and fn(s2=999) == ARG
        assert fn(c=-1) == ARG and fn(c=9) == ARG and fn(K=1, c=1) == ARG
        assert fn(K=0, c=0) == UNSUPPORTED and fn(K=-3, c=0) == UNSUPPORTED and fn(K=33, c=4) == UNSUPPORTED
        assert fn(N=(1 << 24) + 1) == UNSUPPORTED and fn(B=65536) == UNSUPPORTED
        assert fn(ws=A0 + 8) == ARG and fn(ws=B0) == ARG                      # the workspace inside a row block
    # solve
    assert solve(ws=None) == ARG
    for k in range(3):
        assert solve(outs=[None if i == k else o for i, o in enumerate((W1, W2, W3))]) == ARG, k
    assert solve(B=0) == ARG and solve(nc=0) == ARG and solve(c=-1) == ARG and solve(c=9) == ARG
    assert solve(K=0, c=0) == UNSUPPORTED and solve(K=33) == UNSUPPORTED and solve(B=65536) == UNSUPPORTED
    assert solve(nc=(1 << 13) + 1) == UNSUPPORTED
    for v in BAD_RIDGE:
        assert solve(ridge=v) == ARG, v
    for v in BAD_EPS:
        assert solve(eps=v) == ARG, v
    for v in BAD_MAX_GAIN:
        assert solve(max_gain=v) == ARG, v
    assert solve(outs=(W0, W2, W3)) == ARG and solve(outs=(W1, W0 + 16, W3)) == ARG and solve(outs=(W1, W2, W0 + 4)) == ARG
    assert solve(outs=(W1, W1 + 8, W3)) == ARG                                # two outputs on each other
    # apply
    assert apply(x=None) == ARG and apply(taps=None) == ARG and apply(z=None) == ARG
    assert apply(B=0) == ARG and apply(N=0) == ARG and apply(s1=999) == ARG and apply(sz=999) == ARG
    assert apply(c=-1) == ARG and apply(c=9) == ARG
    assert apply(K=0, c=0) == UNSUPPORTED and apply(K=33) == UNSUPPORTED
    assert apply(N=(1 << 24) + 1) == UNSUPPORTED and apply(B=65536) == UNSUPPORTED
    # z may not overlap x (4 rows of 1000 floats from A0 end at A0 + 16000) nor the taps
    assert apply(z=A0) == ARG and apply(z=A0 + 15996) == ARG and apply(x=A0 + 15996, z=A0) == ARG and apply(taps=B0 + 400) == ARG
    # bwd_solve
    for k in range(4):
        assert bwd_solve(ins=[None if i == k else v for i, v in enumerate((W0, W2, W1, W3))]) == ARG, k
    assert bwd_solve(outs=(None, W5)) == ARG and bwd_solve(outs=(W4, None)) == ARG
    assert bwd_solve(B=0) == ARG and bwd_solve(nc=0) == ARG
    assert bwd_solve(K=0) == UNSUPPORTED and bwd_solve(K=33) == UNSUPPORTED and bwd_solve(B=65536) == UNSUPPORTED
    for v in BAD_RIDGE:
        assert bwd_solve(ridge=v) == ARG, v
    for v in BAD_EPS:
        assert bwd_solve(eps=v) == ARG, v
    for k, inp in enumerate((W0, W2, W1, W3)):
        assert bwd_solve(outs=(inp, W5)) == ARG and bwd_solve(outs=(W4, inp)) == ARG, k
    assert bwd_solve(outs=(W4, W4 + 8)) == ARG
    # bwd_apply
    assert bwd_apply(dz=None) == ARG and bwd_apply(y=None) == ARG and bwd_apply(y_hat=None) == ARG and bwd_apply(out=None) == ARG
    for k in range(3):
        assert bwd_apply(small=[None if i == k else v for i, v in enumerate((W1, W4, W5))]) == ARG, k
    assert bwd_apply(B=0) == ARG and bwd_apply(N=0) == ARG and bwd_apply(c=-1) == ARG and bwd_apply(c=9) == ARG
    for k in range(4):
        assert bwd_apply(s=[999 if i == k else None for i in range(4)]) == ARG, k
    assert bwd_apply(K=0, c=0) == UNSUPPORTED and bwd_apply(K=33) == UNSUPPORTED
    assert bwd_apply(N=(1 << 24) + 1) == UNSUPPORTED and bwd_apply(B=65536) == UNSUPPORTED
    # dy_hat may overlap nothing that is read -- dz itself included: there is no in-place update
    assert bwd_apply(out=A0) == ARG and bwd_apply(out=B0) == ARG and bwd_apply(out=C0) == ARG and bwd_apply(out=C0 + 15996) == ARG
    assert bwd_apply(out=A0, s=(1001, None, None, None)) == ARG
    for k in range(3):
        assert bwd_apply(small=[D0 + 64 if i == k else v for i, v in enumerate((W1, W4, W5))]) == ARG, k


def fake_match(B=3, K=9):
    from mod_extraction_amd import fir_match as F
    return F.FirMatch(torch.zeros(B, 48), torch.zeros(B, K), torch.zeros(B, 2 * K + 1, dtype=torch.float64),
                      torch.zeros(B, dtype=torch.int32))


def test_wrapper_errors_are_raised_before_the_launch(monkeypatch):
    from mod_extraction_amd import _hip, fir_match as F
    calls = []
    monkeypatch.setattr(_hip, "call", lambda name, *a: calls.append(name))
    a, b = torch.zeros(3, 48), torch.zeros(3, 48)
    fake = fake_match()
    for fn in (lambda u, v: F.match_fir(u, v), lambda u, v: F.match_fir_backward(a, u, v, fake, 1e-6, 1e-8, 4), F.MatchFir()):
        with pytest.raises(ValueError, match="no CPU fallback"):
            fn(a, b)                                                          # CPU tensors
        with pytest.raises(ValueError, match="fp32"):
            fn(a.double(), b)
        with pytest.raises(ValueError, match="fp32"):
            fn(torch.zeros(3, 2, 48), b)                                     # (B, C, N) with C != 1
        with pytest.raises(ValueError, match="fp32"):
            fn(torch.zeros(48), b)
        with pytest.raises(ValueError, match="fp32"):
            fn([0.0] * 48, b)
    for bad in (0, 33, -1, 9.0, "9", None, True):
        with pytest.raises(ValueError, match="taps"):
            F.match_fir(a, b, taps=bad)
        with pytest.raises(ValueError, match="taps"):
            F.MatchFir(taps=bad)
        with pytest.raises(ValueError, match="taps"):
            F.check_fir(bad, None, 1e-6, 1e-8, 20.0, "x")
    with pytest.raises(TypeError):                                            # ridge, eps and centre have no defaults in the backward
        F.match_fir_backward(a, a, b, fake)
    with pytest.raises(ValueError, match="centre"):                            # and None is not a centre there
        F.match_fir_backward(a, a, b, fake, 1e-6, 1e-8, None)
    for bad in (-1, 9, 4.0, "4", True):
        with pytest.raises(ValueError, match="centre"):
            F.match_fir(a, b, taps=9, centre=bad)
        with pytest.raises(ValueError, match="centre"):
            F.match_fir_backward(a, a, b, fake, 1e-6, 1e-8, bad)
        with pytest.raises(ValueError, match="centre"):
            F.MatchFir(9, centre=bad)
    for bad in (-1e-9, math.inf, math.nan, "0", None, True):
        with pytest.raises(ValueError, match="ridge"):
            F.match_fir(a, b, ridge=bad)
        with pytest.raises(ValueError, match="ridge"):
            F.match_fir_backward(a, a, b, fake, bad, 1e-8, 4)
        with pytest.raises(ValueError, match="ridge"):
            F.MatchFir(ridge=bad)
    for bad in (0.0, -1e-8, math.inf, math.nan, "1e-8", None, True):
        with pytest.raises(ValueError, match="eps"):
            F.match_fir(a, b, eps=bad)
        with pytest.raises(ValueError, match="eps"):
            F.match_fir_backward(a, a, b, fake, 1e-6, bad, 4)
        with pytest.raises(ValueError, match="eps"):
            F.MatchFir(eps=bad)
    for bad in (0.5, 0.0, math.inf, math.nan, "20", None, True):
        with pytest.raises(ValueError, match="max_gain"):
            F.match_fir(a, b, max_gain=bad)
        with pytest.raises(ValueError, match="max_gain"):
            F.MatchFir(max_gain=bad)
    assert F.check_fir(9, None, 0, 1e-8, 1, "x") == (9, 4, 0.0, 1e-8, 1.0) and F.check_fir(8, None, 0.0, 1, 20, "x")[1] == 3
    assert F.check_fir(1, None, 1e-6, 1e-8, 20.0, "x")[:2] == (1, 0) and F.check_fir(32, 31, 1e-6, 1e-8, 20.0, "x")[:2] == (32, 31)
    mod = F.MatchFir(5)
    assert (mod.taps, mod.centre, mod.ridge, mod.eps, mod.max_gain, mod.last) == (5, 2, 1e-6, 1e-8, 20.0, None)
    assert calls == []
    assert F.n_chunks(1) == 1 and F.n_chunks(F.CHUNK) == 1 and F.n_chunks(F.CHUNK + 1) == 2


def test_wrapper_shape_and_overlap_errors(monkeypatch):
    """The checks behind the device check, on CPU tensors that say they are on a HIP device."""
    from mod_extraction_amd import _hip, fir_match as F
    calls = []
    monkeypatch.setattr(_hip, "call", lambda name, *a: calls.append(name))
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    a, b, d = torch.zeros(3, 48), torch.zeros(3, 48), torch.zeros(3, 48)
    fake = fake_match()
    with pytest.raises(ValueError, match="same rows"):
        F.match_fir(a, torch.zeros(3, 47))
    with pytest.raises(ValueError, match="same rows"):
        F.match_fir(a, torch.zeros(2, 48))
    with pytest.raises(ValueError, match="y must be an fp32"):
        F.match_fir(a, b.to(torch.int32))
    with pytest.raises(ValueError, match="no rows"):
        F.match_fir(torch.zeros(0, 48), torch.zeros(0, 48))
    for bad in (torch.zeros(3, 47), torch.zeros(3, 48, dtype=torch.float64), torch.zeros(3, 1, 48), [0.0]):
        with pytest.raises(ValueError, match="out must be"):
            F.match_fir(a, b, out=bad)
    with pytest.raises(ValueError, match="inner stride"):
        F.match_fir(a, b, out=torch.zeros(3, 96)[:, ::2])
    for bad in (a, b):
        with pytest.raises(ValueError, match="overlap"):
            F.match_fir(a, b, out=bad)
    big = torch.zeros(3, 100)
    with pytest.raises(ValueError, match="overlap"):
        F.match_fir(big[:, :48], b, out=big[:, 50:98])                        # interleaved rows of one buffer
    with pytest.raises(ValueError, match="dz must"):
        F.match_fir_backward(torch.zeros(3, 47), a, b, fake, 1e-6, 1e-8, 4)
    with pytest.raises(ValueError, match="FirMatch"):
        F.match_fir_backward(d, a, b, (a, a, a, a), 1e-6, 1e-8, 4)
    with pytest.raises(ValueError, match="match\\.taps"):
        F.match_fir_backward(d, a, b, F.FirMatch(a, torch.zeros(3), fake.sums, fake.flags), 1e-6, 1e-8, 4)
    for k, bad in ((1, torch.zeros(2, 9)), (1, torch.zeros(3, 9, dtype=torch.float64)), (2, torch.zeros(3, 18, dtype=torch.float64)),
                   (2, torch.zeros(3, 19)), (3, torch.zeros(3)), (3, torch.zeros(2, dtype=torch.int32))):
        m = list(fake)
        m[k] = bad
        with pytest.raises(ValueError, match="match\\."):
            F.match_fir_backward(d, a, b, F.FirMatch(*m), 1e-6, 1e-8, 4)
    for dz_, out_ in ((d, d), (d, a), (d, b), (big[:, 50:98], big[:, :48])):   # out=dz is refused too
        with pytest.raises(ValueError, match="no in-place"):
            F.match_fir_backward(dz_, a, b, fake, 1e-6, 1e-8, 4, out=out_)
    assert calls == []
    monkeypatch.setattr(_hip, "stream", lambda: 0)
    # what passes every check launches three times
    out = torch.zeros(3, 48)
    assert F.match_fir_backward(d, a, b, fake, 1e-6, 1e-8, 4, out=out) is out
    assert calls == ["mx_fir_match_bwd_partials", "mx_fir_match_bwd_solve", "mx_fir_match_bwd_apply"]
    del calls[:]
    m = F.match_fir(a.view(3, 1, 48), b.view(3, 1, 48), 5, centre=0)
    assert calls == ["mx_fir_match_partials", "mx_fir_match_solve", "mx_fir_match_apply"]
    assert m._fields == ("z", "taps", "sums", "flags") and m.z.shape == (3, 1, 48) and m.taps.shape == (3, 5)
    assert m.taps.dtype == torch.float32 and m.sums.shape == (3, 11) and m.sums.dtype == torch.float64
    assert m.flags.shape == (3,) and m.flags.dtype == torch.int32


def test_constructor_errors_and_defaults(monkeypatch):
    from mod_extraction_amd import _hip, lightning
    calls = []
    monkeypatch.setattr(_hip, "call", lambda name, *a: calls.append(name))
    mk = lambda **kw: lightning.LFOExtractionThroughEffect(torch.nn.Identity(), **kw)
    plain = mk()
    assert plain.match_fir is None and plain.match_fir_centre is None and plain.step_metric_names == []
    assert (plain.match_fir_ridge, plain.match_fir_eps, plain.match_fir_max_gain) == (1e-6, 1e-8, 20.0)
    step = mk(match_fir=9)
    assert step.match_fir == 9 and step.match_fir_centre == 4 and step.step_metric_names == ["fir/dc_gain", "fir/l1", "fir/flagged"]
    assert mk(match_fir=8).match_fir_centre == 3 and mk(match_fir=8, match_fir_centre=7).match_fir_centre == 7
    assert list(step.state_dict()) == list(plain.state_dict()) and list(step.parameters()) == []      # nothing registered
    assert [n for n, _ in step.named_modules()] == [n for n, _ in plain.named_modules()]
    both = mk(match_fir=5, learned_fx={"flanger": {"mix": {"min": 0.0, "max": 1.0, "init": 0.5}}})
    assert both.step_metric_names == ["fx/flanger.mix", "fir/dc_gain", "fir/l1", "fir/flagged"]
    for mode in ("ls", "rms"):
        with pytest.raises(ValueError, match="mutually exclusive"):
            mk(match_fir=9, match_gain=mode)
    for bad in (0, 33, -1, 9.0, "9", True):
        with pytest.raises(ValueError, match="taps"):
            mk(match_fir=bad)
    for bad in (-1, 9, 4.0):
        with pytest.raises(ValueError, match="centre"):
            mk(match_fir=9, match_fir_centre=bad)
    for bad in (-1, 4.0, "4", True):
        with pytest.raises(ValueError, match="centre"):
            mk(match_fir_centre=bad)                                          # validated without match_fir too
    for kw in ({}, {"match_fir": 9}):
        for bad in (-1e-9, math.nan, "x"):
            with pytest.raises(ValueError, match="ridge"):
                mk(match_fir_ridge=bad, **kw)
        for bad in (0.0, -1.0, math.nan, "x"):
            with pytest.raises(ValueError, match="eps"):
                mk(match_fir_eps=bad, **kw)
        for bad in (0.5, math.inf, "x"):
            with pytest.raises(ValueError, match="max_gain"):
                mk(match_fir_max_gain=bad, **kw)
    assert calls == []


def test_shipped_config():
    """train_lfo_pairs_flanger_fir.yml is train_lfo_pairs_flanger_aligned.yml plus ``match_fir: 9``, and its window stays
    below the flanger's smallest delay (identifiability)."""
    import yaml
    from mod_extraction_amd import cli, lightning
    load = lambda name: yaml.safe_load(open(os.path.join(ROOT, "configs", name)))
    new, base = load("train_lfo_pairs_flanger_fir.yml"), load("train_lfo_pairs_flanger_aligned.yml")
    assert new["model"]["init_args"].pop("match_fir") == 9
    assert new == base
    old = os.getcwd()
    os.chdir(os.path.join(ROOT, "scripts"))
    try:
        mk = lambda name: cli.CustomLightningCLI(args=["fit", "-c", f"../configs/{name}"], run=False, device=torch.device("cpu"))
        c, b = mk("train_lfo_pairs_flanger_fir.yml"), mk("train_lfo_pairs_flanger_aligned.yml")
    finally:
        os.chdir(old)
    assert isinstance(c.model, lightning.LFOExtractionThroughEffect)
    assert c.model.match_fir == 9 and c.model.match_fir_centre == 4 and c.model.match_gain is None and b.model.match_fir is None
    assert c.model.step_metric_names == b.model.step_metric_names + ["fir/dc_gain", "fir/l1", "fir/flagged"]
    assert c.config["data"] == b.config["data"]
    assert {k: v for k, v in c.config["model"]["init_args"].items() if k != "match_fir"} == b.config["model"]["init_args"]
    fixed = new["model"]["init_args"]["learned_fx"]["flanger"]["min_delay_width"]
    assert isinstance(fixed, float)                                           # fixed, not learned
    smallest = fixed * c.model.max_min_delay_samples
    assert c.model.match_fir - 1 - c.model.match_fir_centre < smallest
