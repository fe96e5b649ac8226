"""The route table of the CNN stack node (mod_extraction_amd.models.plan_stack) and the launches that follow from it.

plan_stack is pure (configuration + module knobs -> one BlockRoute per block), so most of this file asserts the table itself.
The launch-name tests run Spectral2DCNN.forward / backward on CPU tensors with the three functions through which the node
reaches the device (_hip.call, _hip.ptr, _hip.stream) replaced by a recorder, inside the test only: every buffer of the node
is a torch.empty, so nothing but the launches is missing.  No GPU needed.
"""
import pytest
import torch

from mod_extraction_amd import _hip, models
from mod_extraction_amd.models import BlockRoute, plan_stack

SHIPPED = dict(cin0=2, dilations=(1, 1, 2, 4, 8, 16), precision="f16x3", n_frames=345)
KNOBS = ["BLOCK1_F16", "WGRAD_SPARSE", "DGRAD_SPARSE", "DIRECT_GRADS", "STATS_FUSED", "GPOOL_FUSED", "LN_FUSED", "BLOCK1_PAIR"]

# Reading the table: block 3 (dilation 4) runs the f16x3 forward on statistics from block 2's epilogue, receives its gradient
# from block 4 as the pooled channels-last pair (block 4's ln_bwd is "gpool"), runs the sparse weight and data gradients and
# hands block 2 a pooled pair in turn.
SHIPPED_TABLE = (
    BlockRoute(fwd="kvec", stats="sweep", leaves_stats=True, g_in="pair", operand="kept", wgrad="kvec_pair",
               routed_pair=False, dgrad=None, ln_bwd=None),
    BlockRoute(fwd="f16x3", stats="epilogue", leaves_stats=True, g_in="pooled", operand="kept", wgrad="sparse",
               routed_pair=False, dgrad="sparse+ln", ln_bwd="pair"),
    BlockRoute(fwd="f16x3", stats="epilogue", leaves_stats=True, g_in="pooled", operand="kept", wgrad="sparse",
               routed_pair=False, dgrad="sparse+ln", ln_bwd="gpool"),
    BlockRoute(fwd="f16x3", stats="epilogue", leaves_stats=True, g_in="pooled", operand="kept", wgrad="sparse",
               routed_pair=False, dgrad="sparse+ln", ln_bwd="gpool"),
    BlockRoute(fwd="f16x3", stats="epilogue", leaves_stats=True, g_in="f32+gmax", operand="kept", wgrad="dense",
               routed_pair=True, dgrad="sparse+ln", ln_bwd="gpool"),
    BlockRoute(fwd="f16x3", stats="epilogue", leaves_stats=False, g_in="f32+gmax", operand="kept", wgrad="dense",
               routed_pair=True, dgrad="sparse+ln", ln_bwd="plain+gmax"),
)


def diff(table, base=SHIPPED_TABLE):
    """{(block, field): value in `table`} for every field that differs from `base`."""
    assert len(table) == len(base)
    return {(l, f): getattr(r, f) for l, (r, b) in enumerate(zip(table, base)) for f in BlockRoute._fields
            if getattr(r, f) != getattr(b, f)}


def fields(blocks, **values):
    return {(l, f): v for l in blocks for f, v in values.items()}


def test_all_knobs_default_on():
    assert all(getattr(models, k) is True for k in KNOBS) and models.WGRAD_SPARSE_MAX_T == 4


def test_shipped_configuration():
    table = plan_stack(**SHIPPED)
    assert table == SHIPPED_TABLE
    assert table[0].fwd == "kvec" and table[0].wgrad == "kvec_pair"
    for r in table[1:4]:
        assert (r.wgrad, r.dgrad, r.g_in, r.routed_pair) == ("sparse", "sparse+ln", "pooled", False)
    for r in table[4:]:
        assert r.wgrad == "dense" and r.dgrad_sparse and r.routed_pair
    assert [r.stats for r in table] == ["sweep"] + ["epilogue"] * 5


# what each knob, switched off alone, changes in the shipped table -- and nothing else
KNOB_OFF = {
    "BLOCK1_F16": {**fields([0], fwd="f32", leaves_stats=False, g_in="f32", operand=None, wgrad="f32"),
                   **fields([1], stats="sweep", ln_bwd="plain")},
    "WGRAD_SPARSE": {**fields([1, 2, 3], wgrad="dense", routed_pair=True, g_in="f32+gmax"),
                     **fields([2, 3, 4], ln_bwd="plain+gmax")},
    "DGRAD_SPARSE": {**fields([1, 2, 3, 4, 5], dgrad="dense"), **fields([1, 2, 3], routed_pair=True),
                     **fields([1, 2, 3, 4], ln_bwd="plain+gmax"), **fields([0, 1, 2, 3], g_in="f32+gmax"),
                     **fields([0], wgrad="kvec_scaled")},
    "DIRECT_GRADS": {},            # where the parameter gradients are written, not which kernels run
    "STATS_FUSED": {**fields([0, 1, 2, 3, 4], leaves_stats=False), **fields([1, 2, 3, 4, 5], stats="sweep")},
    "GPOOL_FUSED": {**fields([2, 3, 4], ln_bwd="plain+gmax"), **fields([1, 2, 3], g_in="f32+gmax")},
    "LN_FUSED": {**fields([1, 2, 3, 4, 5], dgrad="sparse"), **fields([1, 2, 3, 4], ln_bwd="plain+gmax"),
                 **fields([0, 1, 2, 3], g_in="f32+gmax"), **fields([0], wgrad="kvec_scaled")},
    "BLOCK1_PAIR": {**fields([1], ln_bwd="plain+gmax"), **fields([0], g_in="f32+gmax", wgrad="kvec_scaled")},
}


@pytest.mark.parametrize("knob", KNOBS)
def test_each_knob_off_changes_exactly_its_fields(knob, monkeypatch):
    monkeypatch.setattr(models, knob, False)              # read when the table is planned, not at import
    assert diff(plan_stack(**SHIPPED)) == KNOB_OFF[knob]


def test_sparse_weight_gradient_dilation_limit(monkeypatch):
    monkeypatch.setattr(models, "WGRAD_SPARSE_MAX_T", 1)
    assert diff(plan_stack(**SHIPPED)) == {**fields([2, 3], wgrad="dense", routed_pair=True, g_in="f32+gmax"),
                                           **fields([3, 4], ln_bwd="plain+gmax")}


def test_full_pitch_takes_the_dense_kernels():
    table = plan_stack(**{**SHIPPED, "n_frames": 352})
    assert diff(table) == {**fields([1, 2, 3], wgrad="dense", routed_pair=True), **fields([1, 2, 3, 4, 5], dgrad="dense"),
                           **fields([1, 2, 3, 4], ln_bwd="plain+gmax"), **fields([0, 1, 2, 3], g_in="f32+gmax"),
                           **fields([0], wgrad="kvec_scaled")}
    assert all(r.wgrad == "dense" and r.dgrad == "dense" and r.routed_pair for r in table[1:])


F32_BLOCK = dict(fwd="f32", stats="sweep", leaves_stats=False, g_in="f32", operand=None, wgrad="f32", routed_pair=False)


def test_dilated_first_block_takes_fp32_for_that_block_only():
    table = plan_stack(2, (2, 4, 1), "f16x3", 87)
    assert table[0] == BlockRoute(**F32_BLOCK, dgrad=None, ln_bwd=None)
    assert table[1] == BlockRoute(fwd="f16x3", stats="sweep", leaves_stats=True, g_in="pooled", operand="kept", wgrad="sparse",
                                  routed_pair=False, dgrad="sparse+ln", ln_bwd="plain")
    assert table[2] == BlockRoute(fwd="f16x3", stats="epilogue", leaves_stats=False, g_in="f32+gmax", operand="kept",
                                  wgrad="sparse", routed_pair=False, dgrad="sparse+ln", ln_bwd="gpool")


@pytest.mark.parametrize("dilations", [(1, 1, 2, 4, 8, 16), (2, 4, 1), (1,)])
def test_f32_precision_takes_fp32_everywhere(dilations):
    table = plan_stack(2, dilations, "f32", 345)
    assert table[0] == BlockRoute(**F32_BLOCK, dgrad=None, ln_bwd=None)
    assert all(r == BlockRoute(**F32_BLOCK, dgrad="f32", ln_bwd="plain") for r in table[1:])
    assert table == plan_stack(2, dilations, "f32", 345, operands_kept=False)


def test_second_backward_rederives_operands_and_block0_takes_fp32():
    """operands_kept=False (a backward that finds the forward's operand pairs consumed) overrides exactly this."""
    assert diff(plan_stack(**SHIPPED, operands_kept=False)) == {
        **fields([1, 2, 3, 4, 5], operand="rederived"), **fields([0], operand=None, wgrad="f32", g_in="f32"),
        **fields([1], ln_bwd="plain")}


# ---------------------------------------------------------------------------------------------
# launch names
# ---------------------------------------------------------------------------------------------
@pytest.fixture
def launches(monkeypatch):
    """Record (name, *args) of every launch; ptr(t) = (buffer number by first appearance, byte offset, shape, dtype)."""
    log, keep, numbers = [], [], {}

    def ptr(t):
        if t is None:
            return None
        keep.append(t)                                        # no address is ever reused
        base = t.untyped_storage().data_ptr()
        return (numbers.setdefault(base, len(numbers)), t.data_ptr() - base, tuple(t.shape), str(t.dtype))

    monkeypatch.setattr(_hip, "ptr", ptr)
    monkeypatch.setattr(_hip, "call", lambda name, *args: log.append((name, *args)))
    monkeypatch.setattr(_hip, "stream", lambda: 0)
    return log


def shipped_model():
    m = models.Spectral2DCNN(in_ch=2, n_samples=88200, n_mels=64, kernel_size=(5, 13), out_channels=[64] * 6,
                             temp_dilations=[1, 1, 2, 4, 8, 16], pool_size=(2, 1), latent_dim=1, use_ln=True)
    assert not m.generic and m.n_frames == 345
    m.conv_precision = "f16x3"
    return m.eval()


F16_FWD = ["mx_plane_stats_finish", "mx_conv_prep_fwd_f16", "mx_conv_pack_weights_f16", "mx_conv_block_fwd_f16"]
FORWARD = ["mx_logmel_fwd", "mx_plane_stats", "mx_conv_prep_fwd_kvec_f16", "mx_conv_pack_weights_kvec_f16",
           "mx_conv_block1_fwd_f16"] + F16_FWD * 5 + ["mx_head_fwd"]
HEAD_BWD = ["mx_head_bwd"] + ["mx_reduce_rows"] * 3            # head weight, head bias, last PReLU slope
SPARSE_D = ["mx_conv_pack_weights_sp_f16", "mx_conv_block_dgrad_sp_f16"]
# per block: bias reduction first, the slope reduction of the block below last
BACKWARD = {
    5: ["mx_plane_sum", "mx_reduce_rows", "mx_conv_prep_dgrad_f16", "mx_conv_prep_gpool_cl_f16", "mx_conv_block_wgrad_f16",
        *SPARSE_D, "mx_ln_prelu_bwd", "mx_reduce_rows"],
    4: ["mx_reduce_rows", "mx_conv_prep_dgrad_f16", "mx_conv_prep_gpool_cl_f16", "mx_conv_block_wgrad_f16",
        *SPARSE_D, "mx_ln_bwd_finish", "mx_ln_prelu_bwd_gpool_f16", "mx_reduce_rows"],
    3: ["mx_reduce_rows", "mx_conv_block_wgrad_sp_f16", *SPARSE_D, "mx_ln_bwd_finish", "mx_ln_prelu_bwd_gpool_f16",
        "mx_reduce_rows"],
    2: ["mx_reduce_rows", "mx_conv_block_wgrad_sp_f16", *SPARSE_D, "mx_ln_bwd_finish", "mx_ln_prelu_bwd_gpool_f16",
        "mx_reduce_rows"],
    1: ["mx_reduce_rows", "mx_conv_block_wgrad_sp_f16", *SPARSE_D, "mx_ln_bwd_finish", "mx_ln_prelu_bwd_pair",
        "mx_reduce_rows"],
    0: ["mx_reduce_rows", "mx_conv_block1_wgrad_pair_f16"],
}
# the same blocks when the forward's operand pairs are gone: derived again in front of each weight gradient; block 1 hands block 0
# plain fp32 and block 0 runs the exact-fp32 weight gradient
SECOND_BACKWARD = {
    **{l: names[:names.index("mx_conv_block_wgrad_f16")] + ["mx_conv_prep_fwd_f16"] + names[names.index("mx_conv_block_wgrad_f16"):]
       for l, names in BACKWARD.items() if l >= 4},
    **{l: ["mx_reduce_rows", "mx_conv_prep_fwd_f16"] + names[1:] for l, names in BACKWARD.items() if l in (2, 3)},
    1: ["mx_reduce_rows", "mx_conv_prep_fwd_f16", "mx_conv_block_wgrad_sp_f16", *SPARSE_D, "mx_ln_prelu_bwd", "mx_reduce_rows"],
    0: ["mx_reduce_rows", "mx_conv_block_wgrad"],
}


def flat(per_block):
    return HEAD_BWD + [name for l in range(5, -1, -1) for name in per_block[l]]


def test_launch_names_of_the_shipped_configuration(launches):
    m = shipped_model()
    out, lat = m(torch.zeros(2, 2, 88200), (0, 0, 0, 0))
    assert [e[0] for e in launches] == FORWARD
    del launches[:]
    (out.sum() + lat.sum()).backward()
    assert [e[0] for e in launches] == flat(BACKWARD)
    assert launches[-1][0] == "mx_conv_block1_wgrad_pair_f16"


def test_second_backward_through_a_retained_graph(launches):
    m = shipped_model()
    out, lat = m(torch.zeros(2, 2, 88200), (0, 0, 0, 0))
    (out.sum() + lat.sum()).backward(retain_graph=True)
    del launches[:]
    (out.sum() + lat.sum()).backward()
    names = [e[0] for e in launches]
    assert names == flat(SECOND_BACKWARD)
    assert names.count("mx_conv_prep_fwd_f16") == 5 and names[-1] == "mx_conv_block_wgrad"


def test_recorder_is_confined_to_the_test():
    with pytest.raises(_hip.HipLibraryError):               # the product keeps raising for CPU tensors
        _hip.ptr(torch.zeros(1))
