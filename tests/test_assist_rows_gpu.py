"""Speculative decoding with per-row acceptance on the MI355X: `dw_decode_step_rows` (csrc/decode.hip) against the uniform pass and
the float64 per-kernel statement, `dw_assist_pick_rows` / `dw_assist_accept_rows` (csrc/assist.hip) against the numpy restatement on
planted rounds, the device rounds of `assisted_greedy_decode(per_row=True)` against its torch rounds (DW_ASSIST_TORCH=1) and against
every row decoded alone by plain greedy decoding, and `PseudoLabeller(assistant_model=)`.

The rows pass against the uniform pass (`dw_debug_set(7, 12)`: the unfused launch sequence).  For every row b the uniform pass
runs at t = row_t[b] on a copy of the same cache.  Embedding, LayerNorm and the QKV GEMM of layer 0 see identical inputs, so the
K/V the rows pass appends in layer 0 equal the uniform pass's bit for bit.  From layer 1 on the projection's input has passed
through the self-attention, where the rows pass runs its own kernel with its own summation order: those K/V rows are compared
within 2^-6 of the layer's largest value (a few bf16 ulps), and the append itself is checked bit for bit at the LAST layer against
the pass's own QKV workspace.  Cache rows outside [row_t[b], row_t[b] + n) must keep the random values they were filled with.

Logits: max |rows pass - float64| <= LOGIT_FACTOR x max |uniform pass - float64| on the same inputs, the float64 figure being the
per-kernel statement `engine.decode_multi_rows` over oracle.ref_ops in float64 (the same bf16 weights and cache values).  Both
figures are printed.  One different summation order in one kernel would justify a factor of 2; measured on the MI355X over all the
cases below the ratio lies between 0.973 and 1.037 (equal to 1.000 in 14 of 18: the largest deviation of either pass is bf16
rounding of the residual stream and the logits, far from the attention), so the bound is tightened to 1.25.

Key counts: the kernel sweeps 128 keys per step (4 groups of 32 key slots) and its softmax strides a wave (64): a single key,
31 / 32 / 33, 63 / 64 / 65, 127 / 128 / 129 keys and the last cache position.

Near ties in the decoding tests follow tests/test_assist_gpu.py (see tests/test_assist_rows.py)."""
import dataclasses

import numpy as np
import pytest
import torch

from oracle import gen_golden_decode as gd
from oracle.ref_ops import RefOps
from tests import assist_cases as ac
from tests import assist_rows_cases as arc
from tests.assist_rows_restatement import accept_rows_ref, pick_rows_ref
from tests.test_assist_rows import EXACT_ULPS, LENS, compare_with_plain, selected

pytestmark = pytest.mark.gpu
LOGIT_FACTOR = 1.25


@pytest.fixture(scope="module")
def ops():
    from distil_whisper_amd.ops_hip import HipOps
    return HipOps("cuda:0")


# ---- dw_decode_step_rows ---------------------------------------------------------------------------------------------------------
def _pair_of_engines(ops, dims, seed):
    """The bf16 engine on the kernels and the float64 statement over the same (bf16-rounded) weights."""
    from distil_whisper_amd import student_init as si
    from distil_whisper_amd.engine import ParamStore, WhisperEngine
    from distil_whisper_amd.modeling import WhisperForConditionalGeneration
    sd = {k: v.to(torch.bfloat16).float() for k, v in si.random_state_dict(dims, seed, ops.device).items()}
    model = WhisperForConditionalGeneration(dims, ops=ops, state_dict=sd, dtype=torch.bfloat16)
    ref = RefOps("cuda:0", lowp=torch.float64)
    eng64 = WhisperEngine(ref, ParamStore(ref, dims, sd, trainable=False), torch.float64)
    return model.engine, eng64


def _fresh(cache, selfs, t=0):
    return {"B": cache["B"], "max_len": cache["max_len"], "t": t, "cross": cache["cross"], "self": [s.clone() for s in selfs]}


def check_rows_pass(ops, eng, eng64, B, n, row_t, max_len, seed):
    d = eng.dims
    D, dev = d.d_model, ops.device
    g = torch.Generator().manual_seed(seed)
    enc = (torch.randn(B * d.max_src, D, generator=g) * 0.5).to(dev).to(torch.bfloat16)
    ids = torch.randint(0, d.vocab, (B, n), generator=g).to(dev)
    cache = eng.decode_init(enc, B, max_len)
    base = [(torch.randn(B * max_len, 2 * D, generator=g) * 0.5).to(dev).to(torch.bfloat16) for _ in cache["self"]]
    for kv, b0 in zip(cache["self"], base):
        kv.copy_(b0)                                       # history below row_t, and the sentinel everywhere else
    rt = torch.tensor(row_t, dtype=torch.int32, device=dev)
    assert ops.lib.dw_debug_set(7, 12) == 0
    try:
        got = eng.decode_multi_rows(ids, cache, rt, max(row_t)).view(B, n, -1)[:, :, :d.vocab].float().clone()
        qkv_last = cache[("desc", n)][1]["qkv"].clone()
        uni = torch.empty_like(got)
        uni_kv = []
        for b, t in enumerate(row_t):
            c2 = _fresh(cache, base, t)
            uni[b] = eng.decode_multi(ids, c2).view(B, n, -1)[b, :, :d.vocab].float()
            uni_kv.append([s.view(B, max_len, 2 * D)[b, t:t + n].clone() for s in c2["self"]])
    finally:
        ops.lib.dw_debug_set(7, 4)
    torch.cuda.synchronize()
    # ---- the cache: written rows and untouched rows
    for l, (kv, b0) in enumerate(zip(cache["self"], base)):
        kv3, b3 = kv.view(B, max_len, 2 * D), b0.view(B, max_len, 2 * D)
        for b, t in enumerate(row_t):
            keep = torch.ones(max_len, dtype=torch.bool, device=dev)
            keep[t:t + n] = False
            assert torch.equal(kv3[b][keep], b3[b][keep]), f"layer {l} row {b}: a cache row outside [t, t + n) changed"
            w, u = kv3[b, t:t + n], uni_kv[b][l]
            if l == 0:
                assert torch.equal(w, u), f"layer 0 row {b}: appended K/V differ from the uniform pass"
            else:
                diff = (w.float() - u.float()).abs().max().item()
                assert diff <= u.float().abs().max().item() * 2.0 ** -6, (l, b, diff)
    last = cache["self"][-1].view(B, max_len, 2 * D)
    for b, t in enumerate(row_t):
        assert torch.equal(last[b, t:t + n], qkv_last[b * n:(b + 1) * n, D:]), f"row {b}: the last layer's append is not a copy"
    # ---- logits against the float64 statement
    c64 = eng64.decode_init(enc.double(), B, max_len)
    for kv, b0 in zip(c64["self"], base):
        kv.copy_(b0.double())
    ref = eng64.decode_multi_rows(ids, c64, rt, max(row_t)).view(B, n, -1)[:, :, :d.vocab]
    dev_rows = (got.double() - ref).abs().max().item()
    dev_uni = (uni.double() - ref).abs().max().item()
    print(f"B {B} n {n} row_t {row_t}: max |logits - f64|: rows pass {dev_rows:.4e}, uniform pass {dev_uni:.4e}, "
          f"ratio {dev_rows / dev_uni:.3f}")
    assert dev_uni > 0 and dev_rows <= LOGIT_FACTOR * dev_uni
    return dev_rows / dev_uni


@pytest.fixture(scope="module")
def tiny(ops):
    from distil_whisper_amd.engine import WhisperDims
    return _pair_of_engines(ops, dataclasses.replace(WhisperDims.from_any(gd.CFG_T), max_src=128), 3)


@pytest.mark.parametrize("n", [1, 2, 6])
def test_rows_pass_against_the_uniform_pass_tiny(ops, tiny, n):
    eng, eng64 = tiny
    max_len = 160
    for i, row_t in enumerate(([0, 64 - n, max_len - n], [31 - n, 32 - n, 33 - n], [63 - n, 64 - n, 65 - n],
                               [127 - n, 128 - n, 129 - n], [5, 0, 70])):
        check_rows_pass(ops, eng, eng64, 3, n, row_t, max_len, 100 * n + i)


@pytest.fixture(scope="module")
def wide(ops):
    from distil_whisper_amd.engine import WhisperDims
    return _pair_of_engines(ops, WhisperDims(1280, 20, 5120, 1, 2, 51866, 128, max_src=128), 5)


@pytest.mark.parametrize("B", [2, 6, 11])
def test_rows_pass_against_the_uniform_pass_at_distil_large_v3_width(ops, wide, B):
    """D = 1280, 20 heads, 2 layers, n = 6: 12 rows (LayerNorm inside the GEMM), 36 (past it), 66 (past the uniform pass's fused
    K/V append as well)."""
    eng, eng64 = wide
    row_t = [0, 100, 37, 64, 122, 1, 63, 58, 99, 31, 12][:B]
    check_rows_pass(ops, eng, eng64, B, 6, row_t, 128, 40 + B)


def test_rows_pass_rejects_bad_arguments_without_a_launch(ops, tiny):
    import ctypes as C
    eng, _ = tiny
    d, dev = eng.dims, ops.device
    B, n, max_len = 3, 2, 64
    enc = torch.zeros((B * d.max_src, d.d_model), dtype=torch.bfloat16, device=dev)
    cache = eng.decode_init(enc, B, max_len)
    desc, ws, _, _ = eng._decode_desc(cache, n)
    ids = torch.zeros((B, n), dtype=torch.long, device=dev)
    desc.ids = ids.data_ptr()
    rt = torch.zeros(B, dtype=torch.int32, device=dev)
    for t in list(ws.values()) + cache["self"]:
        t.fill_(3.0)
    s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    call = ops.lib.dw_decode_step_rows
    assert call(C.byref(desc), None, 10, s) == -1                          # null row_t
    assert call(C.byref(desc), rt.data_ptr(), max_len - n + 1, s) == -1    # max_t + n > max_len
    assert call(C.byref(desc), rt.data_ptr(), -1, s) == -1
    assert call(C.byref(desc), rt.data_ptr() + 2, 10, s) == -1             # misaligned
    assert call(None, rt.data_ptr(), 10, s) == -1
    torch.cuda.synchronize()
    assert all(bool((t == 3.0).all()) for t in list(ws.values()) + cache["self"])
    assert call(C.byref(desc), rt.data_ptr(), max_len - n, s) == 0         # the largest bound that fits
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ws["logits"][:, :d.vocab].float()).all())


# ---- dw_assist_pick_rows / dw_assist_accept_rows -----------------------------------------------------------------------------------
def device_round(ops, c, ld):
    """One verify round through the two entries -> (own, tokens, lens, done, pos_t, pos_a, result) as numpy / lists."""
    dev = ops.device
    B, n, V = c["logits"].shape
    k = c["k"]
    rows = n + 2                                           # the pass scored more rows than the k + 1 that are read
    lg = torch.full((B * rows, ld), 50.0, dtype=torch.bfloat16, device=dev)        # (pad columns / rows would win if read)
    lg.view(B, rows, ld)[:, 2:, :V] = torch.from_numpy(c["logits"]).to(dev).to(torch.bfloat16)
    tokens = torch.from_numpy(c["tokens"]).to(dev)
    own = torch.full((B, n + 1), -5, dtype=torch.long, device=dev)
    done = torch.from_numpy(c["done"]).to(dev)
    length = torch.tensor(c["lens"], dtype=torch.int32, device=dev)
    pos_t, pos_a = (torch.full((B,), -7, dtype=torch.int32, device=dev) for _ in range(2))
    result = torch.full((4,), -9, dtype=torch.int32, device=dev)
    sup = None
    if c["suppress"]:
        sup = torch.zeros(V, dtype=torch.uint8, device=dev)
        sup[torch.tensor(c["suppress"], device=dev)] = 1
    ts = c["ts"]
    ops.assist_pick_rows(lg[2:], V, tokens, length, own, n=n, batch_rows=rows, suppress=sup, min_new=c["min_new"],
                         ts_begin=-1 if ts is None else ts["no_timestamps_token_id"] + 1,
                         max_initial=-1 if ts is None else ts["max_initial_timestamp_index"], begin_index=c["P0"], eos=c["eos"])
    ops.assist_accept_rows(own, tokens, length, k, c["total"], result, done, pos_t, pos_a, eos=c["eos"], fill=c["fill"])
    torch.cuda.synchronize()
    assert (own[:, n:] == -5).all()
    return (own.cpu().numpy(), tokens.cpu().numpy(), length.tolist(), done.tolist(), pos_t.tolist(), pos_a.tolist(), result.tolist())


@pytest.mark.parametrize("V,ld", [(1030, 1032), (51865, 51872), (51866, 51868), (53252, 53312)])
def test_kernels_match_the_restatement_on_planted_rounds(ops, V, ld):
    from tests.test_assist_rows import check_round
    small = V < 2000
    for k in ((0, 1, 5) if small else (5,)):
        for name in ac.scenarios(3, k):
            if not small and name not in ("rows_differ", "done_row", "eos_accepted", "min_new_inside", "suppress", "ts_first",
                                          "ts_text_ts", "ts_pair", "ts_open", "ts_mass_taken", "ts_mass_not_taken"):
                continue
            c = arc.planted_rows(V, LENS, k, name)
            check_round(device_round(ops, c, ld), c, (V, k, name))


def test_a_row_at_total_stays_in_bounds(ops):
    c = arc.planted_rows(1030, LENS, 5, "all_accepted")
    c["lens"] = [7, c["total"], c["total"] - 1]
    c["min_new"], c["suppress"], c["ts"] = 0, [], None
    own_ref, _ = pick_rows_ref(c["logits"], c["tokens"], c["lens"], 0, c["P0"], c["eos"], 0, (), (), None)
    ref = accept_rows_ref(own_ref, c["tokens"], c["lens"], 5, c["total"], c["done"], c["eos"], c["fill"])
    own, tokens, lens, done, pos_t, pos_a, result = device_round(ops, c, 1032)
    assert own[:, :6].tolist() == own_ref.tolist() and tokens.tolist() == ref[0].tolist()
    assert (lens, done, pos_t, pos_a, result) == (ref[1].tolist(), ref[2].tolist(), ref[3].tolist(), ref[4].tolist(), ref[5])


def test_pick_rows_at_one_length_equals_assist_pick(ops):
    dev = ops.device
    for V, ld in ((1030, 1032), (51866, 51868)):
        for name in ("rows_differ", "suppress", "min_new_inside", "ts_first", "ts_text_ts", "ts_pair", "ts_open", "ts_mass_taken"):
            for k in (0, 5):
                c = arc.planted_rows(V, [8, 8, 8], k, name)
                L = c["lens"][0]                           # (3 for the scenario of the first generated position)
                n, ts = k + 1, c["ts"]
                lg = torch.zeros((3 * n, ld), dtype=torch.bfloat16, device=dev)
                lg[:, :V] = torch.from_numpy(c["logits"]).to(dev).to(torch.bfloat16).view(3 * n, V)
                sup = None
                if c["suppress"]:
                    sup = torch.zeros(V, dtype=torch.uint8, device=dev)
                    sup[torch.tensor(c["suppress"], device=dev)] = 1
                kw = dict(n=n, suppress=sup, min_new=c["min_new"], ts_begin=-1 if ts is None else ts["no_timestamps_token_id"] + 1,
                          max_initial=-1 if ts is None else ts["max_initial_timestamp_index"], begin_index=c["P0"], eos=c["eos"])
                tokens = torch.from_numpy(c["tokens"]).to(dev)
                own1, own2 = (torch.full((3, n), -1, dtype=torch.long, device=dev) for _ in range(2))
                ops.assist_pick(lg, V, tokens, L, own1, **kw)
                ops.assist_pick_rows(lg, V, tokens, torch.full((3,), L, dtype=torch.int32, device=dev), own2, **kw)
                assert torch.equal(own1, own2) and own1.tolist() == c["own"].tolist(), (V, name, k)
        # the draft step: the same token at tokens[:, L + j0] and in cur
        c = ac.make_case(5, V, 3, 0, ac.scenarios(3, 0)["all_accepted"])
        lg = torch.zeros((3, ld), dtype=torch.bfloat16, device=dev)
        lg[:, :V] = torch.from_numpy(c["logits"][:, 0]).to(dev).to(torch.bfloat16)
        L = c["L"]
        t1 = torch.from_numpy(np.concatenate([c["tokens"], np.full((3, 4), 7)], 1)).to(dev)
        t2 = t1.clone()
        cur1, cur2 = (torch.zeros((3, 1), dtype=torch.long, device=dev) for _ in range(2))
        own1, own2 = (torch.zeros((3, 1), dtype=torch.long, device=dev) for _ in range(2))
        ops.assist_pick(lg, V, t1, L + 2, own1, n=1, begin_index=c["P0"], eos=c["eos"], store=True, cur=cur1)
        ops.assist_pick_rows(lg, V, t2, torch.full((3,), L, dtype=torch.int32, device=dev), own2, n=1, j0=2, begin_index=c["P0"],
                             eos=c["eos"], store=True, cur=cur2)
        assert torch.equal(t1, t2) and torch.equal(cur1, cur2) and torch.equal(own1, own2)


# ---- the rounds through assisted_greedy_decode ---------------------------------------------------------------------------------
def _run(monkeypatch, torch_path, target, assistant, enc, prompt, max_new, K, spy=False, **kw):
    """-> (rows, drafted, accepted, per-round gains of live rows, smallest margin in bf16 ulps [torch path with spy], calls)."""
    from distil_whisper_amd import decoding
    from tests.test_assist_rows import run_rows
    monkeypatch.setenv(decoding.ASSIST_TORCH_ENV, "1" if torch_path else "0")
    if torch_path:
        out = run_rows(monkeypatch, target, assistant, enc, prompt, max_new, K, **kw)
        monkeypatch.undo()
        return out
    calls, gains = {}, []
    for name in ("assist_pick_rows", "assist_accept_rows", "decode_pass_rows"):
        fn = getattr(type(target.ops), name)

        def counted(self, *a, _fn=fn, _name=name, **k2):
            calls[_name] = calls.get(_name, 0) + 1
            if _name == "assist_accept_rows":
                before, was = a[2].tolist(), a[6].tolist()
                _fn(self, *a, **k2)
                gains.append([n - o for n, o, w in zip(a[2].tolist(), before, was) if not w])
                return None
            return _fn(self, *a, **k2)
        monkeypatch.setattr(type(target.ops), name, counted)
    ids, drafted, accepted = decoding.assisted_greedy_decode(target.engine, assistant.engine, enc, enc, prompt, max_new, K,
                                                             per_row=True, **kw)
    monkeypatch.undo()
    return ids.tolist(), drafted, accepted, gains, None, calls


def compare_paths(monkeypatch, cases, prompt, max_new, K, pad, **kw):
    """cases: (target, assistant, enc, plain) per input.  Kernel rounds against torch rounds on the inputs without an exactly tied
    selection, and against `plain(enc)` -- every row decoded alone -- where every margin exceeds EXACT_ULPS."""
    tried = same = exact = 0
    results = []
    for target, assistant, enc, plain in cases:
        tried += 1
        want = _run(monkeypatch, True, target, assistant, enc, prompt, max_new, K, **kw)
        margin = want[4]
        print(f"input {tried}: smallest margin {margin:.1f} ulps")
        if margin <= 0.0:
            continue
        got = _run(monkeypatch, False, target, assistant, enc, prompt, max_new, K, **kw)
        print(f"  drafted {got[1]}, accepted {got[2]}, gains {got[3]}, calls {got[5]}")
        assert got[:4] == want[:4]
        assert all(got[5].get(n, 0) > 0 for n in ("assist_pick_rows", "assist_accept_rows", "decode_pass_rows"))
        same += 1
        if margin > EXACT_ULPS:
            compare_with_plain(got[0], plain(enc), pad)
            exact += 1
            results.append(got)
    selected(tried, same)
    selected(tried, exact)
    return results


def _planted(ops, sd, cfg, P, seq, weak, row_tokens, max_src, scale=1.0, head_gain=1.0):
    from distil_whisper_amd.engine import WhisperDims
    from distil_whisper_amd.modeling import WhisperForCausalLM, WhisperForConditionalGeneration
    d = WhisperDims.from_any(cfg)
    sd = {k: v.cpu() for k, v in sd.items()}
    sd_t, sd_a, enc = arc.planted_pair(sd, P, seq, weak, row_tokens, d.d_model, max_src, scale, head_gain=head_gain)
    target = WhisperForConditionalGeneration(cfg, ops=ops, state_dict=sd_t, dtype=torch.bfloat16)
    assistant = WhisperForCausalLM(cfg, ops=ops, state_dict={k: v for k, v in sd_a.items() if k.startswith("model.decoder.")},
                                   dtype=torch.bfloat16)
    return target, assistant, enc.to(ops.device).to(torch.bfloat16)


def _plain(target, prompt, max_new, eos, suppress, rules, min_new):
    from distil_whisper_amd.decoding import GreedyDecoder
    d = target.dims
    dec = GreedyDecoder(target.engine, 1, prompt.shape[1] + max_new, eos_token_id=eos, suppress_tokens=suppress, pad_token_id=eos,
                        timestamp_rules=rules, use_graphs=False)
    return lambda enc: [dec.run(enc[b * d.max_src:(b + 1) * d.max_src].contiguous(), prompt[b:b + 1].contiguous(), max_new,
                                min_new_tokens=min_new)[0].tolist() for b in range(prompt.shape[0])]


@pytest.mark.parametrize("timestamps", [False, True])
@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("K", [1, 5])
def test_kernel_rounds_equal_torch_rounds_and_every_row_alone_tiny(ops, monkeypatch, timestamps, B, K):
    """tests/assist_rows_cases.planted_pair on the tiny model of the decode fixtures: row 0 accepts every draft, row 1 rejects at
    the weak steps, row 2 (B = 3) rejects at the strong ones and ends at its own EOS at the first weak step."""
    fields = gd.generation_fields(multilingual=True, suppress=True, timestamps=timestamps)
    ids = [gd.SOT, gd.LANG["<|en|>"], gd.TRANSCRIBE] + ([] if timestamps else [gd.NOTIMESTAMPS])
    P, eos, max_new, T0 = len(ids), gd.EOS, 8, gd.TS0
    seq = [T0 + 1, 50, 61, T0 + 5, T0 + 5, 72, T0 + 9, eos] if timestamps else [50, 61, 72, 83, 94, 105, eos, 116]
    weak = (2, 5)
    row_tokens = [400, 410, eos][:B]
    prompt = torch.tensor([ids] * B, device=ops.device)
    rules = dict(begin_index=P, no_timestamps_token_id=gd.NOTIMESTAMPS, max_initial_timestamp_index=50) if timestamps else None
    kw = dict(eos_token_id=eos, suppress_tokens=fields["suppress_tokens"], min_new_tokens=2, pad_token_id=eos, timestamp_rules=rules)
    cases = []
    for seed in (77, 78, 79):                              # (on the CPU statement in bf16 every margin of these is >= 24 ulps)
        target, assistant, enc = _planted(ops, gd.weights(seed), gd.CFG_T, P, seq, weak, row_tokens, gd.CFG_T.max_src, scale=4.0, head_gain=4.0)
        cases.append((target, assistant, enc, _plain(target, prompt, max_new, eos, fields["suppress_tokens"], rules, 2)))
    for rows, drafted, accepted, gains, _, _ in compare_paths(monkeypatch, cases, prompt, max_new, K, eos, **kw):
        want = arc.expected_rows(seq, weak, row_tokens, eos, max_new)
        assert [r[P:P + len(w)] for r, w in zip(rows, want)] == want
        assert any(len(set(g)) > 1 for g in gains), "every row accepted alike in every round"
        assert 0 < accepted < drafted


def test_kernel_rounds_equal_torch_rounds_at_distil_large_v3_width(ops, monkeypatch):
    """d_model 1280, V = 51 866, a 4-layer target and its planted twin, 8 new tokens, K = 5, B = 3, no EOS among the row tokens:
    every row runs to the budget, at its own pace."""
    from distil_whisper_amd import student_init as si
    from distil_whisper_amd.engine import WhisperDims
    d = WhisperDims(1280, 20, 5120, 1, 4, 51866, 128, max_src=256)
    B, eos, P = 3, 50257, 3
    seq = [1000, 2000, 3000, 4000, 5000, 6000, 7000, 8000]
    weak, row_tokens = (1, 4, 6), [1500, 2500, 3500]
    target, assistant, enc = _planted(ops, si.random_state_dict(d, 5, ops.device), d, P, seq, weak, row_tokens, d.max_src, scale=10.0)
    prompt = torch.tensor([[50258, 50259, 50360]] * B, device=ops.device)
    kw = dict(eos_token_id=eos, min_new_tokens=1, pad_token_id=eos)
    cases = [(target, assistant, enc, _plain(target, prompt, 8, eos, None, None, 1))]
    for rows, drafted, accepted, gains, _, _ in compare_paths(monkeypatch, cases, prompt, 8, 5, eos, **kw):
        assert [r[P:] for r in rows] == arc.expected_rows(seq, weak, row_tokens, eos, 8)
        assert any(len(set(g)) > 1 for g in gains) and 0 < accepted < drafted


# ---- PseudoLabeller(assistant_model=) ------------------------------------------------------------------------------------------
def test_pseudo_labeller_with_an_assistant_returns_the_labels_without_one(ops, monkeypatch):
    """The fixture audio through the tiny teacher with peaked positions (tests/test_assist_gpu.peaked: the encoder output of real
    features enters every layer) and its decoder-only student, which disagrees at two steps; also under overlap=True."""
    from distil_whisper_amd import decoding
    from distil_whisper_amd.modeling import WhisperFeatureExtractor, WhisperForCausalLM, WhisperForConditionalGeneration
    from distil_whisper_amd.pseudo_label import PseudoLabeller
    from tests.test_assist_gpu import peaked
    fields = gd.generation_fields(multilingual=True, suppress=True, timestamps=False)
    prompt = [gd.SOT, gd.LANG["<|en|>"], gd.TRANSCRIBE, gd.NOTIMESTAMPS]
    P, eos = len(prompt), gd.EOS
    seq_t = [50, 61, 72, 83, 94, 105, eos, 116]
    seq_s = list(seq_t)
    seq_s[2], seq_s[5] = 400, 401
    sd_t = gd.weights(77)
    sd_s, cfg_s = gd.student(peaked(sd_t, P, seq_s, 100.0))
    teacher = WhisperForConditionalGeneration(gd.CFG_T, ops=ops, state_dict=peaked(sd_t, P, seq_t, 100.0), dtype=torch.bfloat16)
    causal = WhisperForCausalLM(cfg_s, ops=ops, state_dict=sd_s, dtype=torch.bfloat16)
    fe = WhisperFeatureExtractor(feature_size=80, ops=ops)
    kw = dict(batch_size=2, max_new_tokens=8, prompt_ids=prompt, eos_token_id=eos, suppress_tokens=fields["suppress_tokens"],
              begin_suppress_tokens=fields["begin_suppress_tokens"])
    tried = exact = 0
    for seed in (3, 4):
        audios = [gd.audio(seed * 10 + i, n) for i, n in enumerate((150_000, 200_000, 100_000, 300_000))]
        speakers = (0, 0, 0, 1)
        tried += 1
        want, packs, _ = PseudoLabeller(teacher, fe, **kw)(audios, speakers)
        margins = []
        orig = decoding.assist_pick_torch

        def spy(logits, *a, **k2):
            own = orig(logits, *a, **k2)
            lg = logits.float()
            best = lg.gather(-1, own[..., None])
            second = orig(lg.scatter(-1, own[..., None], float("-inf")), *a, **k2)
            gap = (best - lg.gather(-1, second[..., None]))[..., 0]
            margins.append((gap / torch.exp2(torch.floor(torch.log2(best[..., 0].abs().clamp(min=1e-30))) - 7)).min().item())
            return own
        monkeypatch.setenv(decoding.ASSIST_TORCH_ENV, "1")
        monkeypatch.setattr(decoding, "assist_pick_torch", spy)
        on_torch, _, _ = PseudoLabeller(teacher, fe, assistant_model=causal, num_assistant_tokens=3, **kw)(audios, speakers)
        monkeypatch.undo()
        print(f"audio seed {seed}: packs {packs}, smallest margin {min(margins):.1f} ulps")
        if min(margins) <= 0.0:
            continue
        for overlap in (False, True):
            got, packs2, _ = PseudoLabeller(teacher, fe, assistant_model=causal, num_assistant_tokens=3, overlap=overlap, **kw)(
                audios, speakers)
            assert packs2 == packs and got == on_torch
        if min(margins) > EXACT_ULPS:
            assert got == want and all(row == seq_t[:seq_t.index(eos)] for row in got)
            exact += 1
    selected(tried, exact)
