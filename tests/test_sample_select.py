"""Sampled decoding in the selection kernel (`dw_sample_select`, csrc/decode.hip), the part that needs no GPU: the numpy
restatement of the entry (tests/sample_restatement.py) against tests/golden/sample_select.json -- tokens that `transformers`'
processors, warpers and `torch.multinomial` produced (tools/gen_golden_sample_select.py) --, the premise the entry rests on
(one multinomial draw per row is argmax(probs / Exponential(1) noise) and consumes the generator alike), the C entry's argument
checks, and the decoder's choice of path.

Every comparison is token for token: the fixture holds no row within the restatement's "near" margins (the generator rejects them,
and the test below asserts the fixture's rejection count against the issue's cap of 2 %)."""
import ctypes

import numpy as np
import pytest
import torch

import sample_restatement as sr

GOLD = sr.gold()
SC = {s["name"]: s for s in GOLD["scenarios"]}


def inputs(sc):
    """-> (logits f32 [B, V], noise f32 [B, V], tokens int64 [B, ld], done bool [B], keyword arguments with the masks as uint8 [V])"""
    B, V = sc["B"], sc["V"]
    kw = dict(sc["kwargs"])
    for k in ("suppress", "begin_suppress"):
        if kw[k] is not None:
            m = np.zeros(V, dtype=np.uint8)
            m[kw[k]] = 1
            kw[k] = m
    return (sr.bf16_unpack(sc["logits_bf16"], (B, V)), sr.f32_unpack(sc["noise_f32"], (B, V)), np.array(sc["tokens"], dtype=np.int64),
            np.array(sc["done"], dtype=bool), kw)


def test_fixture_covers_every_rule_and_state():
    assert GOLD["drawn"] >= sum(s["B"] for s in SC.values()) and GOLD["rejected"] <= 0.02 * GOLD["drawn"]
    assert all(s["V"] <= 2048 and s["B"] <= 3 for s in SC.values())
    kw = {n: s["kwargs"] for n, s in SC.items()}
    assert kw["temperature"]["top_k"] == 0 and kw["temperature"]["top_p"] == 1.0 and kw["temperature"]["temperature"] != 1.0
    assert kw["top_k"]["top_k"] > 1 and kw["top_k_1"]["top_k"] == 1 and kw["top_p"]["top_p"] < 1.0
    assert kw["top_k_top_p"]["top_k"] > 0 and kw["top_k_top_p"]["top_p"] < 1.0
    assert kw["repetition_penalty"]["repetition_penalty"] != 1.0 and kw["no_repeat_ngram"]["no_repeat_ngram"] == 2
    assert kw["suppress"]["suppress"] and kw["first_begin_suppress"]["begin_suppress"] and kw["first_begin_suppress"]["first"]
    assert kw["no_eos"]["no_eos"] and SC["finished_row"]["done"] == [0, 1, 0]
    for name in ("ts_first", "ts_closed_pair", "ts_text_timestamp", "ts_mass_fires", "ts_mass_quiet", "top_k_beyond_allowed"):
        assert kw[name]["ts_begin"] > 0
    assert kw["ts_first"]["first"] and kw["ts_first"]["max_initial"] == 50
    both = kw["all_together"]
    assert both["repetition_penalty"] != 1.0 and both["no_repeat_ngram"] and both["suppress"] and both["ts_begin"] > 0 and \
        both["top_k"] > 0 and both["top_p"] < 1.0 and SC["all_together"]["V"] > SC["temperature"]["V"] and \
        SC["all_together"]["B"] == 3 and SC["all_together_b1"]["B"] == 1
    # the states are what their names say, in the reference's own tokens
    for name, sc in SC.items():
        tb, eos = sc["kwargs"]["ts_begin"], sc["kwargs"]["eos"]
        live = [t for t, d in zip(sc["expected"], sc["done"]) if not d]
        if name in ("ts_first", "ts_mass_fires"):
            assert all(t >= tb for t in live), name
        if name in ("ts_closed_pair", "ts_mass_quiet"):
            assert all(t < tb for t in live), name
        if name in ("ts_text_timestamp", "top_k_beyond_allowed"):
            assert all(t >= tb or t == eos for t in live), name
        if name in ("no_eos", "all_together_b1"):
            assert eos not in live, name
    assert SC["finished_row"]["expected"][1] == SC["finished_row"]["kwargs"]["fill"]
    # more columns asked for than are allowed: top-k removes nothing
    sc = SC["top_k_beyond_allowed"]
    logits, noise, tokens, done, k = inputs(sc)
    for b in range(sc["B"]):
        s, _ = sr.processed_row(logits[b], tokens[b, :sc["n"]].tolist(), tokens[b, k["begin_index"]:sc["n"]].tolist(), sc["V"],
                                **{x: k[x] for x in ("ts_begin", "max_initial", "eos")})
        assert 0 < np.isfinite(s).sum() < k["top_k"]
        assert np.isfinite(sr.warp_row(s, k["temperature"], k["top_k"])[0]).sum() == np.isfinite(s).sum()


@pytest.mark.parametrize("name", sorted(SC))
def test_restatement_reproduces_the_reference_tokens(name):
    sc = SC[name]
    logits, noise, tokens, done, kw = inputs(sc)
    nxt, new_done, margins = sr.sample_select_ref(logits, noise, sc["V"], tokens, sc["n"], done=done, **kw)
    assert nxt.tolist() == sc["expected"]
    assert new_done.astype(int).tolist() == sc["expected_done"]
    assert not (sr.near(margins) & ~done).any(), margins


def test_restatement_margins_and_the_boundary_group():
    # two equal scores straddle the boundary: whole, the group stays; split, its first member (in sort order) goes
    s = np.log(np.array([0.1, 0.3, 0.3, 0.3], dtype=np.float64)).astype(np.float32)
    whole, dist = sr.warp_row(s, top_p=0.55)              # budget 0.45: mass(<= 0.3-group) = 1.0, mass(<= 0.1) = 0.1
    assert np.isfinite(whole).tolist() == [False, True, True, True] and dist == pytest.approx(0.35, abs=1e-6)
    split, _ = sr.warp_row(s, top_p=0.55, split_groups=True)
    assert np.isfinite(split).tolist() == [False, False, True, True]
    # ties at the top-k threshold stay; fewer finite scores than k: nothing goes
    t = np.array([1.0, 3.0, 2.0, 2.0, -np.inf], dtype=np.float32)
    assert np.isfinite(sr.warp_row(t, top_k=2)[0]).tolist() == [False, True, True, True, False]
    assert np.isfinite(sr.warp_row(t, top_k=5)[0]).tolist() == [True, True, True, True, False]
    # the draw: equal quotients go to the smaller column, no column at all gives 0
    col, gap = sr.draw_row(np.zeros(4, dtype=np.float32), np.array([2.0, 1.0, 1.0, 4.0], dtype=np.float32))
    assert col == 1 and gap == 0.0
    assert sr.draw_row(np.full(4, -np.inf, dtype=np.float32), np.ones(4, dtype=np.float32)) == (0, np.inf)
    near = sr.near(dict(quotient=np.array([1e-5, 1.0, 1.0, 1.0]), boundary=np.array([1.0, 1e-6, 1.0, 1.0]),
                        mass=np.array([1.0, 1.0, 1e-4, 1.0])))
    assert near.tolist() == [True, True, True, False]


@pytest.mark.parametrize("B", [1, 3, 16])
def test_one_multinomial_draw_is_argmax_of_probs_over_exponential_noise(B):
    """the premise of the kernel: same token, same generator state afterwards, also with half the columns at probability 0"""
    V = 51866
    g0 = torch.Generator().manual_seed(100 + B)
    mismatches = 0
    for trial in range(6):
        probs = torch.softmax(torch.randn(B, V, generator=g0) * 3.0, -1)
        if trial % 2:
            probs = probs * (torch.rand(B, V, generator=g0) < 0.5)
            probs = probs / probs.sum(-1, keepdim=True)
        ga, gb = torch.Generator().manual_seed(7 + trial), torch.Generator().manual_seed(7 + trial)
        want = torch.multinomial(probs, 1, generator=ga)[:, 0]
        q = torch.empty_like(probs).exponential_(1.0, generator=gb)
        got = (probs / q).argmax(-1)
        mismatches += int((want != got).sum())
        assert torch.equal(ga.get_state(), gb.get_state())
    assert mismatches == 0


def test_dw_sample_select_is_declared_exported_and_rejects_bad_arguments_without_touching_the_gpu():
    import os
    from distil_whisper_amd import ops_hip
    header = open(os.path.join(os.path.dirname(ops_hip.__file__), "..", "include", "dwamd.h")).read()
    assert "int dw_sample_select(" in header
    assert "dw_sample_select" in ops_hip.EXPORTED_SYMBOLS and hasattr(ops_hip.HipOps, "sample_select")
    lib = ops_hip.load_library()
    good = ctypes.c_void_p(0x10000)                 # never dereferenced: every call below fails validation before any launch

    def call(logits=good, B=2, V=1000, ld=1000, first=0, no_eos=0, ts_begin=-1, max_initial=-1, tokens=good, tok_ld=16, n=4,
             begin=4, eos=900, fill=900, done=good, cur=good, penalty=1.2, ngram=2, temperature=0.8, top_k=50, top_p=0.9,
             noise=good, noise_ld=1000):
        return lib.dw_sample_select(logits, B, V, ld, None, None, first, no_eos, ts_begin, max_initial, tokens, tok_ld, n, begin,
                                    eos, fill, done, cur, penalty, ngram, temperature, top_k, top_p, noise, noise_ld, None)
    assert call(noise=None) == -1 and call(noise_ld=999) == -1 and call(V=65537, ld=65540, noise_ld=65540) == -1
    for t in (0.0, -0.5, float("inf"), float("nan")):
        assert call(temperature=t) == -1, t
    assert call(top_k=-1) == -1
    for p in (0.0, -0.1, 1.5, float("nan")):
        assert call(top_p=p) == -1, p
    # everything dw_greedy_select_history checks
    assert call(logits=None) == -1 and call(tokens=None) == -1 and call(cur=None) == -1 and call(done=None) == -1
    assert call(penalty=0.0) == -1 and call(penalty=float("inf")) == -1 and call(penalty=float("nan")) == -1 and call(ngram=-1) == -1
    assert call(B=0) == -1 and call(n=0) == -1 and call(n=16) == -1 and call(V=0) == -1
    assert call(ld=996) == -1 and call(ld=1002) == -1 and call(logits=ctypes.c_void_p(0x10004)) == -1
    assert call(ts_begin=912, eos=-1) == -1 and call(ts_begin=912, begin=0) == -1 and call(ts_begin=912, begin=5) == -1


def test_decoder_over_ref_ops_keeps_the_torch_path(monkeypatch):
    import history_restatement as hr
    from distil_whisper_amd import decoding
    from oracle import gen_golden_decode as gd
    from oracle.ref_ops import RefOps
    sc = {s["name"]: s for s in hr.gold()["scenarios"]}["both"]
    ops = RefOps("cpu", lowp=torch.float32)
    assert not hasattr(ops, "sample_select")
    eng = hr.dropin(ops, sc).engine
    soft = dict(do_sample=True, temperature=0.8, top_k=50, top_p=0.9, repetition_penalty=1.2, no_repeat_ngram_size=2)
    dec = decoding.GreedyDecoder(eng, 2, 16, eos_token_id=gd.EOS, use_graphs=True, soft=dict(soft))
    assert dec.sample is None and dec.noise is None and dec.history is None and not dec.use_graphs

    # ops with the entry keep the graphs and get the static noise buffer; the switch forces the torch path on them as well
    class WithEntry(RefOps):
        def sample_select(self, *a, **k):
            raise AssertionError("not called here")
    eng2 = hr.dropin(WithEntry("cpu", lowp=torch.float32), sc).engine
    monkeypatch.delenv(decoding.SAMPLE_TORCH_ENV, raising=False)
    dec = decoding.GreedyDecoder(eng2, 2, 16, eos_token_id=gd.EOS, use_graphs=True, soft=dict(soft))
    assert dec.use_graphs and dec.noise.shape == (2, eng2.dims.vocab) and dec.noise.dtype == torch.float32 and dec.noise.is_contiguous()
    assert dec.sample == dict(repetition_penalty=1.2, no_repeat_ngram=2, temperature=0.8, top_k=50, top_p=0.9)
    dec = decoding.GreedyDecoder(eng2, 2, 16, eos_token_id=gd.EOS, use_graphs=True, soft=dict(do_sample=True, temperature=0.5))
    assert dec.sample == dict(repetition_penalty=1.0, no_repeat_ngram=0, temperature=0.5, top_k=0, top_p=1.0)
    monkeypatch.setenv(decoding.SAMPLE_TORCH_ENV, "1")
    dec = decoding.GreedyDecoder(eng2, 2, 16, eos_token_id=gd.EOS, use_graphs=True, soft=dict(soft))
    assert dec.sample is None and not dec.use_graphs
