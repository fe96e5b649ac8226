"""CPU: the surface of the gain match (K20) -- its declarations in include/modex_hip.h against ``_hip.SIGNATURES``, the
limits of the four entry points (checked before any launch, so without a device), the ``ValueError``s of the wrappers in
``mod_extraction_amd.gain`` and of the step's constructor, and the shipped config.  No device work."""
import ctypes
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"mx_gain_match_partials": 8, "mx_gain_match_apply": 16, "mx_gain_match_bwd_partials": 8, "mx_gain_match_bwd_apply": 17}
ARG, UNSUPPORTED = -1, -2
LS, RMS = 0, 1


def test_header_table_and_symbols():
    """Four entry points, declared in include/modex_hip.h (section K20) and bound from ``_hip.SIGNATURES``, which is derived
    from that text; the three ``MX_GAIN_*`` defines of the same section against their Python mirrors."""
    from mod_extraction_amd import _hip, build, gain
    from tests.test_abi import header_arg_counts
    lib = ctypes.CDLL(build.build(verbose=False))
    raw = open(os.path.join(ROOT, "include", "modex_hip.h")).read()
    assert {k: v for k, v in header_arg_counts().items() if k.startswith("mx_gain_match_")} == NAMES
    assert {k: len(v) for k, v in _hip.SIGNATURES.items() if k.startswith("mx_gain_match_")} == NAMES
    assert _hip.ABI_VERSION == 21 == lib.mx_abi_version()
    assert int(re.search(r"^#define MX_GAIN_CHUNK (\d+)$", raw, flags=re.M).group(1)) == gain.CHUNK
    assert gain.CHUNK % 4 == 0 and gain.MODES == ("ls", "rms")
    assert [int(re.search(rf"^#define MX_GAIN_{m.upper()} (\d+)$", raw, flags=re.M).group(1)) for m in gain.MODES] == [LS, RMS]
    zeros = {ctypes.c_void_p: None, ctypes.c_int64: 0, ctypes.c_int32: 0, ctypes.c_float: 0.0, ctypes.c_double: 0.0}
    for name in NAMES:
        assert hasattr(lib, name)
        fn = getattr(_hip.load(), name)
        assert fn.argtypes == _hip.SIGNATURES[name]                           # load() binds the table
        assert fn(*[zeros[t] for t in fn.argtypes]) == ARG


def p(v):
    return None if v is None else ctypes.c_void_p(v)


A0, B0, C0, D0 = 1 << 20, 2 << 20, 3 << 20, 4 << 20                          # four row blocks that are far apart


def partials(y_hat=A0, y=B0, B=4, N=1000, s1=None, s2=None, ws=8):
    from mod_extraction_amd import _hip
    return _hip.load().mx_gain_match_partials(p(y_hat), N if s1 is None else s1, p(y), N if s2 is None else s2, B, N, p(ws), None)


def bwd_partials(dz=A0, y_hat=B0, B=4, N=1000, s1=None, s2=None, ws=8):
    from mod_extraction_amd import _hip
    return _hip.load().mx_gain_match_bwd_partials(p(dz), N if s1 is None else s1, p(y_hat), N if s2 is None else s2, B, N, p(ws),
                                                  None)


def apply(y_hat=A0, ws=8, B=4, N=1000, mode=LS, eps=1e-8, clamp=1, lo=0.05, hi=20.0, z=B0, s1=None, sz=None, outs=(8, 8, 8)):
    from mod_extraction_amd import _hip
    return _hip.load().mx_gain_match_apply(p(y_hat), N if s1 is None else s1, p(ws), B, N, mode, eps, clamp, lo, hi, p(z),
                                           N if sz is None else sz, *[p(o) for o in outs], None)


def bwd_apply(dz=A0, y_hat=B0, y=C0, ins=(8, 8, 8, 8), B=4, N=1000, mode=LS, eps=1e-8, out=D0, s=(None,) * 4):
    from mod_extraction_amd import _hip
    st = [N if v is None else v for v in s]
    return _hip.load().mx_gain_match_bwd_apply(p(dz), st[0], p(y_hat), st[1], p(y), st[2], *[p(i) for i in ins], B, N, mode, eps,
                                               p(out), st[3], None)


def test_limits_are_checked_before_any_launch():
    """Every case is refused on pointers that are never read (a case that would launch is not tried here)."""
    for fn, first, second in ((partials, "y_hat", "y"), (bwd_partials, "dz", "y_hat")):
        assert fn(**{first: None}) == ARG and fn(**{second: None}) == ARG and fn(ws=None) == ARG
        assert fn(B=0) == ARG and fn(B=-2) == ARG and fn(N=0) == ARG and fn(N=-5) == ARG
        assert fn(s1=999) == ARG and fn(s2=999) == ARG
        assert fn(N=(1 << 24) + 1) == UNSUPPORTED and fn(B=65536) == UNSUPPORTED
    assert apply(y_hat=None) == ARG and apply(ws=None) == ARG and apply(z=None) == ARG
    for k in range(3):
        assert apply(outs=[None if i == k else 8 for i in range(3)]) == ARG, k
    assert apply(B=0) == ARG and apply(N=0) == ARG and apply(s1=999) == ARG and apply(sz=999) == ARG
    assert apply(mode=2) == ARG and apply(mode=-1) == ARG
    for eps in (0.0, -1e-8, math.inf, math.nan):
        assert apply(eps=eps) == ARG, eps
    for lo, hi in ((0.0, 20.0), (-0.1, 20.0), (1.5, 20.0), (0.05, 0.9), (0.05, math.inf), (math.nan, 20.0), (0.05, math.nan)):
        assert apply(lo=lo, hi=hi) == ARG, (lo, hi)
    assert apply(N=(1 << 24) + 1) == UNSUPPORTED and apply(B=65536) == UNSUPPORTED
    # z may not overlap y_hat: 4 rows of 1000 floats from A0 end at A0 + 16000
    assert apply(z=A0) == ARG and apply(z=A0 + 15996) == ARG and apply(y_hat=A0 + 15996, z=A0) == ARG
    assert bwd_apply(dz=None) == ARG and bwd_apply(y_hat=None) == ARG and bwd_apply(y=None) == ARG and bwd_apply(out=None) == ARG
    for k in range(4):
        assert bwd_apply(ins=[None if i == k else 8 for i in range(4)]) == ARG, k
    assert bwd_apply(B=0) == ARG and bwd_apply(N=0) == ARG and bwd_apply(mode=2) == ARG and bwd_apply(eps=0.0) == ARG
    for k in range(4):
        assert bwd_apply(s=[999 if i == k else None for i in range(4)]) == ARG, k
    assert bwd_apply(N=(1 << 24) + 1) == UNSUPPORTED and bwd_apply(B=65536) == UNSUPPORTED
    # dy_hat may be dz itself (same pointer, same stride) and nothing else that is read
    assert bwd_apply(out=B0) == ARG and bwd_apply(out=C0) == ARG and bwd_apply(out=A0 + 4) == ARG
    assert bwd_apply(out=A0, s=(1001, None, None, None)) == ARG and bwd_apply(out=C0 + 15996) == ARG


def test_wrapper_errors_are_raised_before_the_launch(monkeypatch):
    from mod_extraction_amd import _hip, gain as G
    calls = []
    monkeypatch.setattr(_hip, "call", lambda name, *a: calls.append(name))
    a, b = torch.zeros(3, 48), torch.zeros(3, 48)
    fake = G.GainMatch(a, torch.zeros(3), torch.zeros(3, 3, dtype=torch.float64), torch.zeros(3, dtype=torch.int32))
    for fn in (lambda u, v: G.match_gain(u, v), lambda u, v: G.match_gain_backward(a, u, v, fake), G.MatchGain()):
        with pytest.raises(ValueError, match="no CPU fallback"):
            fn(a, b)                                                          # CPU tensors
        with pytest.raises(ValueError, match="fp32"):
            fn(a.double(), b)
        with pytest.raises(ValueError, match="fp32"):
            fn(a.to(torch.int32), b)
        with pytest.raises(ValueError, match="fp32"):
            fn(torch.zeros(3, 2, 48), b)                                     # (B, C, N) with C != 1
        with pytest.raises(ValueError, match="fp32"):
            fn(torch.zeros(48), b)
        with pytest.raises(ValueError, match="fp32"):
            fn([0.0] * 48, b)
    for bad in ("l2", "LS", None, 0):
        with pytest.raises(ValueError, match="mode"):
            G.match_gain(a, b, mode=bad)
        with pytest.raises(ValueError, match="mode"):
            G.match_gain_backward(a, a, b, fake, mode=bad)
        with pytest.raises(ValueError, match="mode"):
            G.MatchGain(mode=bad)
    for bad in (0.0, -1e-8, math.inf, math.nan, "1e-8", None, True):
        with pytest.raises(ValueError, match="eps"):
            G.match_gain(a, b, eps=bad)
        with pytest.raises(ValueError, match="eps"):
            G.MatchGain(eps=bad)
    for bad in ((0.0, 20.0), (1.5, 20.0), (0.05, 0.9), (0.05,), (0.05, 1.0, 20.0), 1.0, (0.05, math.inf), (math.nan, 2.0), ("a", 2.0)):
        with pytest.raises(ValueError, match="gain_range"):
            G.match_gain(a, b, gain_range=bad)
        with pytest.raises(ValueError, match="gain_range"):
            G.MatchGain(gain_range=bad)
    assert calls == []
    assert G.n_chunks(1) == 1 and G.n_chunks(G.CHUNK) == 1 and G.n_chunks(G.CHUNK + 1) == 2


def test_wrapper_shape_and_overlap_errors(monkeypatch):
    """The checks behind the device check, on CPU tensors that say they are on a HIP device."""
    from mod_extraction_amd import _hip, gain as G
    calls = []
    monkeypatch.setattr(_hip, "call", lambda name, *a: calls.append(name))
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    a, b, d = torch.zeros(3, 48), torch.zeros(3, 48), torch.zeros(3, 48)
    fake = G.GainMatch(a, torch.zeros(3), torch.zeros(3, 3, dtype=torch.float64), torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="same rows"):
        G.match_gain(a, torch.zeros(3, 47))
    with pytest.raises(ValueError, match="same rows"):
        G.match_gain(a, torch.zeros(2, 48))
    with pytest.raises(ValueError, match="y must be an fp32"):
        G.match_gain(a, b.to(torch.int32))
    with pytest.raises(ValueError, match="no rows"):
        G.match_gain(torch.zeros(0, 48), torch.zeros(0, 48))
    for bad in (torch.zeros(3, 47), torch.zeros(3, 48, dtype=torch.float64), torch.zeros(3, 1, 48), [0.0]):
        with pytest.raises(ValueError, match="out must be"):
            G.match_gain(a, b, out=bad)
    with pytest.raises(ValueError, match="inner stride"):
        G.match_gain(a, b, out=torch.zeros(3, 96)[:, ::2])
    with pytest.raises(ValueError, match="overlap"):
        G.match_gain(a, b, out=a)
    with pytest.raises(ValueError, match="overlap"):
        G.match_gain(a, b, out=b)
    big = torch.zeros(3, 100)
    with pytest.raises(ValueError, match="overlap"):
        G.match_gain(big[:, :48], b, out=big[:, 50:98])                       # interleaved rows of one buffer
    with pytest.raises(ValueError, match="dz must"):
        G.match_gain_backward(torch.zeros(3, 47), a, b, fake)
    with pytest.raises(ValueError, match="GainMatch"):
        G.match_gain_backward(d, a, b, (a, a, a, a))
    for k, bad in ((1, torch.zeros(2)), (1, torch.zeros(3, dtype=torch.float64)), (2, torch.zeros(3, 3)), (3, torch.zeros(3))):
        m = list(fake)
        m[k] = bad
        with pytest.raises(ValueError, match="match\\."):
            G.match_gain_backward(d, a, b, G.GainMatch(*m))
    for dz_, out_ in ((d, a), (d, b), (big[:, 50:98], big[:, :48])):
        with pytest.raises(ValueError, match="out may be dz itself"):
            G.match_gain_backward(dz_, a, b, fake, out=out_)
    assert calls == []
    monkeypatch.setattr(_hip, "stream", lambda: 0)
    # what passes every check launches twice; out=dz is the in-place update
    out = G.match_gain_backward(d, a, b, fake, out=d)
    assert out is d and calls == ["mx_gain_match_bwd_partials", "mx_gain_match_bwd_apply"]
    del calls[:]
    m = G.match_gain(a.view(3, 1, 48), b.view(3, 1, 48), "rms", gain_range=(0.5, 2.0))
    assert calls == ["mx_gain_match_partials", "mx_gain_match_apply"]
    assert m._fields == ("z", "gain", "sums", "flags") and m.z.shape == (3, 1, 48) and m.gain.shape == (3,)
    assert m.sums.shape == (3, 3) and m.sums.dtype == torch.float64 and m.flags.dtype == torch.int32


def test_constructor_errors_and_defaults(monkeypatch):
    from mod_extraction_amd import _hip, lightning
    calls = []
    monkeypatch.setattr(_hip, "call", lambda name, *a: calls.append(name))
    mk = lambda **kw: lightning.LFOExtractionThroughEffect(torch.nn.Identity(), **kw)
    plain = mk()
    assert plain.match_gain is None and plain.step_metric_names == [] and plain.match_gain_range == (0.05, 20.0)
    assert plain.match_gain_eps == 1e-8
    step = mk(match_gain="ls")
    assert step.match_gain == "ls" and step.step_metric_names == ["gain/mean", "gain/std", "gain/clamped"]
    assert list(step.state_dict()) == list(plain.state_dict()) and list(step.parameters()) == []      # nothing registered
    assert [n for n, _ in step.named_modules()] == [n for n, _ in plain.named_modules()]
    both = mk(match_gain="rms", match_gain_range=[0.5, 2.0], learned_fx={"flanger": {"mix": {"min": 0.0, "max": 1.0, "init": 0.5}}})
    assert both.step_metric_names == ["fx/flanger.mix", "gain/mean", "gain/std", "gain/clamped"]
    assert both.match_gain_range == (0.5, 2.0) and mk(match_gain="ls", match_gain_range=None).match_gain_range is None
    for bad in ("l2", "LS", True, 1):
        with pytest.raises(ValueError, match="mode"):
            mk(match_gain=bad)
    for kw in ({}, {"match_gain": "ls"}):
        for bad in (0.0, -1.0, math.nan, "x"):
            with pytest.raises(ValueError, match="eps"):
                mk(match_gain_eps=bad, **kw)
        for bad in ((0.0, 20.0), (2.0, 20.0), (0.05, 0.5), (1.0,), 3.0):
            with pytest.raises(ValueError, match="gain_range"):
                mk(match_gain_range=bad, **kw)
    assert calls == []


def test_shipped_config():
    """train_lfo_pairs_flanger_gain.yml is train_lfo_pairs_flanger_aligned.yml plus ``match_gain: ls``."""
    import yaml
    from mod_extraction_amd import cli, lightning
    load = lambda name: yaml.safe_load(open(os.path.join(ROOT, "configs", name)))
    new, base = load("train_lfo_pairs_flanger_gain.yml"), load("train_lfo_pairs_flanger_aligned.yml")
    assert new["model"]["init_args"].pop("match_gain") == "ls"
    assert new == base
    old = os.getcwd()
    os.chdir(os.path.join(ROOT, "scripts"))
    try:
        mk = lambda name: cli.CustomLightningCLI(args=["fit", "-c", f"../configs/{name}"], run=False, device=torch.device("cpu"))
        c, b = mk("train_lfo_pairs_flanger_gain.yml"), mk("train_lfo_pairs_flanger_aligned.yml")
    finally:
        os.chdir(old)
    assert isinstance(c.model, lightning.LFOExtractionThroughEffect)
    assert c.model.match_gain == "ls" and c.model.match_gain_range == (0.05, 20.0) and c.model.match_gain_eps == 1e-8
    assert b.model.match_gain is None
    assert c.model.step_metric_names == b.model.step_metric_names + ["gain/mean", "gain/std", "gain/clamped"]
    assert c.config["data"] == b.config["data"]
    assert {k: v for k, v in c.config["model"]["init_args"].items() if k != "match_gain"} == b.config["model"]["init_args"]
