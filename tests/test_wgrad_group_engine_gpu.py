"""Engine.group_wgrad: the backward of one encoder layer with its four weight-gradient GEMMs in one grouped launch (dw_wgrad_group)
against the same backward with one split-K launch per matrix, from the same seeded state.

D = 1280, ffn = 5120, 20 heads, 2 x 160 = 320 rows.  Every weight gradient is judged against the float64 product of the (dy, x) the
layer handed to _wgrad, with the bound of tests/test_wgrad_group_gpu.py (that of tests/test_training_kernels_edges_gpu.py::
test_layernorm_width_sweep, dgamma): row_err(grouped, float64) <= F x row_err(RefOps, float64).

Bias gradients.  The group leaves them where they were: the same ops.colsum calls on the same bits into the same targets, which the
test asserts call by call, and the gradients that deterministic kernels form (out_proj.bias, from the LayerNorm backward) are
bit-equal.  fc1.bias and the q / v biases are column sums that dw_colsum_bf16 adds with float atomics, one per block of 16 rows in
arrival order: the same call on the same bits gives other last bits from run to run (seen on the MI355X: fc1.bias, 320 rows), so
bit-equality cannot be asked of them with or without the group; they are held to ATOMIC_ORDER, the figure tests/test_training_kernels_edges_gpu.py keeps
for column sums that group the rows differently.  The fused fc1.bias sums of the dX GEMM (fuse_fc1_bias_grad, float atomics too) are
switched off, so that fc1.bias takes the column-sum path of _wgrad, the one the group touches.
D = 768 (small.en: 768 is no multiple of 320) must take the launches it always took."""
import pytest
import torch

import training_restatement as tr
from guarded import DEV
from test_training_kernels_edges_gpu import ATOMIC_ORDER, F_BOUND

pytestmark = pytest.mark.gpu

F = F_BOUND["dgamma"]
B, L = 2, 160
P = "model.encoder.layers.0"
WEIGHTS = [f"{P}.{n}.weight" for n in ("fc1", "fc2", "self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.out_proj")]
BIASES_EXACT = [f"{P}.{n}.bias" for n in ("fc2", "self_attn.k_proj", "self_attn.out_proj")]      # no float atomics (module docstring)
BIASES_ATOMIC = [f"{P}.{n}.bias" for n in ("fc1", "self_attn.q_proj", "self_attn.v_proj")]
BIASES = BIASES_EXACT + BIASES_ATOMIC


@pytest.fixture(scope="module")
def ops():
    from distil_whisper_amd.ops_hip import HipOps
    return HipOps(DEV)


@pytest.fixture(scope="module")
def ref():
    from oracle.ref_ops import RefOps
    return RefOps(DEV)


def engine(ops, d_model, heads, ffn):
    from distil_whisper_amd.engine import ParamStore, WhisperDims, WhisperEngine
    from oracle import whisper_oracle as wo
    cfg = wo.OracleConfig(d_model, heads, ffn, 1, 1, 1000, 80, max_src=L, max_tgt=8, pad_token_id=0, decoder_start_token_id=1)
    eng = WhisperEngine(ops, ParamStore(ops, WhisperDims.from_any(cfg), wo.init_state_dict(cfg, 11), trainable=True), torch.float32)
    eng.fuse_fc1_bias_grad = False      # (module docstring)
    return eng


def check_biases(on, off, sums_on, sums_off):
    """module docstring, "Bias gradients" """
    assert len(sums_on) == len(sums_off) and len(sums_on) >= 3
    for (x1, out1, acc1), (x2, out2, acc2) in zip(sums_on, sums_off):
        assert torch.equal(x1, x2) and out1 == out2 and acc1 == acc2
    for n in BIASES_EXACT:
        assert torch.equal(on[n], off[n]), n
    for n in BIASES_ATOMIC:
        e = tr.row_err(on[n], off[n], 1)
        print(f"WGRAD_GROUP_LAYER {n} grouped against ungrouped {e:.4e}")
        assert bool(off[n].any()) and e <= ATOMIC_ORDER, (n, e)


def layer_backward(eng, group, overwrite, record=None, sums=None):
    """forward + backward of the layer from seeded inputs -> {name: gradient}; record: receives the (dy, x, gout) handed to _wgrad,
    sums: the (x, address of out, accumulate) of every ops.colsum call"""
    D, R = eng.dims.d_model, B * L
    g = torch.Generator(device=DEV).manual_seed(5)
    x = eng.act(R, D, dtype=torch.float32)
    x[:R] = torch.randn((R, D), generator=g, device=DEV)
    dres = torch.randn((R, D), generator=g, device=DEV) * 0.05
    dy = eng.act(R, D)
    dy[:R] = dres.to(dy.dtype)
    _, lc = eng._layer_fwd(P, x, B, L, None, 0, False, True)
    G = eng.st.G
    G[eng.st.train_start:eng.st.train_end].zero_()
    if overwrite:                      # the weight matrices are stored, whatever they held
        for n in WEIGHTS:
            eng.st.g[n].fill_(float("nan"))
    eng.group_wgrad, eng.wgrad_overwrite = group, overwrite
    inner = eng._wgrad
    if record is not None:
        def spy(dy_, x_, gout, gbias, R_, bias_cols=None):
            if gout is not None:
                record.append((dy_, x_, gout))
            return inner(dy_, x_, gout, gbias, R_, bias_cols)
        eng._wgrad = spy
    colsum = eng.ops.colsum
    if sums is not None:
        def colsum_spy(x_, out, accumulate):
            sums.append((x_.clone(), out.data_ptr(), bool(accumulate)))
            return colsum(x_, out, accumulate)
        eng.ops.colsum = colsum_spy
    try:
        eng._layer_bwd(P, lc, dres.clone(), dy, B, L, 0, False, None, True, None)
        eng._wgrad_fence()
        eng.join_wgrad_stream()
    finally:
        eng.wgrad_overwrite = False
        eng.__dict__.pop("_wgrad", None)
        eng.ops.__dict__.pop("colsum", None)
    torch.cuda.synchronize()
    if record is not None:             # (the gradients are views of the flat buffer, which the next run clears)
        record[:] = [(dy_, x_, gout.clone()) for dy_, x_, gout in record]
    return {n: eng.st.g[n].clone() for n in WEIGHTS + BIASES}


@pytest.mark.parametrize("overwrite", [False, True], ids=["accumulate", "overwrite"])
def test_layer_backward_grouped_equals_one_launch_per_matrix(ops, ref, overwrite):
    eng = engine(ops, 1280, 20, 5120)
    ops.profile = {}
    try:
        handed, handed_off, sums, sums_off = [], [], [], []
        off = layer_backward(eng, False, overwrite, record=handed_off, sums=sums_off)
        keys_off = ops.collect_profile()
        n0 = eng.wgrad_groups_issued
        on = layer_backward(eng, True, overwrite, record=handed, sums=sums)
        keys_on = ops.collect_profile()
    finally:
        ops.profile = None
    # one grouped launch instead of the four launches with both operands k-major
    assert eng.wgrad_groups_issued == n0 + 1 and len(handed) == 4
    assert keys_on["gemm_g320_TT"]["n"] == 1 and not any(k.endswith("_TT") and k != "gemm_g320_TT" for k in keys_on)
    assert "gemm_g320_TT" not in keys_off and sum(v["n"] for k, v in keys_off.items() if k.endswith("_TT")) == 4
    assert keys_on["gemm_g320_TT"]["flops"] == sum(v["flops"] for k, v in keys_off.items() if k.endswith("_TT"))
    # the (dy, x) of the two runs are the same bits (every kernel above them is deterministic), so one float64 product judges both
    for i, ((dy, x, g_on), (dy2, x2, g_off)) in enumerate(zip(handed, handed_off)):
        assert torch.equal(dy, dy2) and torch.equal(x, x2), i
        want64 = dy.double().t() @ x.double()
        want32 = ref.gemm(dy, x, trans_a=True, trans_b=True, out_dtype=torch.float32)
        e_ref = tr.row_err(want32, want64, want64.shape[1])
        e_on, e_off = tr.row_err(g_on, want64, want64.shape[1]), tr.row_err(g_off, want64, want64.shape[1])
        print(f"WGRAD_GROUP_LAYER matrix {i} {tuple(g_on.shape)} grouped {e_on:.4e} split-K {e_off:.4e} ref {e_ref:.4e} "
              f"ratio {e_on / e_ref:.3f}")
        assert bool(torch.isfinite(g_on).all()), i
        assert e_on <= F * e_ref, (i, e_on, e_ref)
        assert e_off <= F * e_ref, (i, e_off, e_ref)
    for n in WEIGHTS:       # (what the optimizer reads: the views of the flat gradient buffer by parameter name)
        assert bool(torch.isfinite(on[n]).all()) and bool(torch.isfinite(off[n]).all()), n
    check_biases(on, off, sums, sums_off)


def test_small_en_width_takes_the_launches_it_always_took(ops):
    eng = engine(ops, 768, 12, 3072)
    ops.profile = {}
    try:
        sums, sums_off = [], []
        off = layer_backward(eng, False, False, sums=sums_off)
        keys_off = ops.collect_profile()
        on = layer_backward(eng, True, False, sums=sums)
        keys_on = ops.collect_profile()
    finally:
        ops.profile = None
    assert eng.wgrad_groups_issued == 0 and "gemm_g320_TT" not in keys_on
    assert {k: v["n"] for k, v in keys_on.items()} == {k: v["n"] for k, v in keys_off.items()}
    for n in WEIGHTS:
        assert torch.equal(on[n], off[n]), n
    check_biases(on, off, sums, sums_off)
