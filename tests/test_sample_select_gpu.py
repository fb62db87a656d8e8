"""Sampled decoding in the selection kernel on the MI355X (`dw_sample_select`, csrc/decode.hip): the kernel against its numpy
restatement (tests/sample_restatement.py) token for token, the fixture scenarios of tests/golden/sample_select.json (expected
tokens from `transformers`) through the kernel, and the decoder / `generate` with the kernel (HIP graphs on and off) against the
torch path (`DW_SAMPLE_TORCH=1`) under one seed, generator state included.

Where the bounds come from: none is needed.  The noise is drawn on the CPU with fixed seeds, so every kernel-level case is decided
by the restatement before the kernel runs; the seeds are such that no row is "near" (a quotient gap below 1e-4, a cumulative mass
within 1e-5 of 1 - top_p, a mass rule within 1e-3 of its threshold -- the restatement's docstring), which each test asserts, and
then a few ulp in `exp` or a division cannot move a token."""
import numpy as np
import pytest
import torch

import history_restatement as hr
import sample_restatement as sr
from oracle import gen_golden_decode as gd

pytestmark = pytest.mark.gpu

GOLD = sr.gold()
P, LD_TOK = 4, 16
# V, ld: Whisper's vocabulary, an odd width (rows of the noise are then not even 8-byte aligned), a micro vocabulary (one chunk
# per thread and a partial one), and one beyond 13 x 4096 columns (the kernel's 16-chunk form)
SHAPES = [(51866, 51904), (51865, 51904), (1030, 1032), (53252, 53312)]
A_, B_, C_ = 101, 202, 405


@pytest.fixture(scope="module")
def ops():
    from distil_whisper_amd.ops_hip import HipOps
    return HipOps("cuda:0")


def _ids(V):
    return V - 100, V - 88                          # eos, first timestamp id (<|notimestamps|> = tb - 1)


def _masks(V):
    eos, tb = _ids(V)
    sup = np.zeros(V, dtype=np.uint8)
    sup[:40] = 1
    sup[300:340] = 1
    sup[eos + 1:tb - 1] = 1
    sup[tb + 50] = 1
    bsup = np.zeros(V, dtype=np.uint8)
    bsup[[220, eos, tb + 1]] = 1
    return sup, bsup


def _modes(V):
    """name -> (generated history of three rows, selection arguments, logit edits)"""
    eos, t = _ids(V)
    sup, bsup = _masks(V)
    text = [[A_, B_, C_, 61, 62], [A_, B_, A_, C_, A_], [61, 62, 63, 64, 65]]
    ts = dict(ts_begin=t, max_initial=50)
    return {
        "temperature": (text, dict(temperature=0.8), {}),
        "top_k=1": (text, dict(temperature=0.9, top_k=1), dict(peak=True)),
        "top_k=50": (text, dict(temperature=1.1, top_k=50), {}),
        "top_p=0.6": (text, dict(temperature=0.7, top_p=0.6), {}),
        "top_k, top_p, penalty, 2-gram": (text, dict(temperature=0.8, top_k=50, top_p=0.6, repetition_penalty=1.3, no_repeat_ngram=2),
                                          dict(plant=[(0, A_, 9.0), (1, B_, 9.0), (1, C_, 8.5)])),
        "top_p, penalty, 2-gram": (text, dict(temperature=0.7, top_p=0.6, repetition_penalty=1.3, no_repeat_ngram=2),
                                   dict(plant=[(0, A_, 9.0), (1, B_, 9.0)])),
        "timestamps: first token": ([[], [], []], dict(temperature=0.8, **ts), {}),
        "timestamps: closed pair": ([[t, 41, t + 5, t + 5], [t + 2, 42, t + 9, t + 9], [t + 1, 43, t + 3, t + 3]],
                                    dict(temperature=0.8, **ts), dict(ts_shift=3.0)),
        "timestamps: text + timestamp": ([[t + 1, 41, t + 9], [t + 1, 41, t + 30], [t + 2, 42, t + 11]],
                                         dict(temperature=0.8, top_k=40, **ts), {}),
        "timestamps: mass rule fires": ([[t + 2, 41, 42], [t + 1, 43, 44], [t + 3, 45, 46]], dict(temperature=0.8, **ts),
                                        dict(ts_shift=9.0)),
        "timestamps: mass rule quiet": ([[t + 2, 41, 42], [t + 1, 43, 44], [t + 3, 45, 46]], dict(temperature=0.8, top_p=0.85, **ts),
                                        dict(ts_shift=-4.0)),
        "first, begin-suppress": ([[], [], []], dict(temperature=1.0, suppress=sup, begin_suppress=bsup),
                                  dict(plant=[(0, 220, 14.0), (1, eos, 14.0)])),
        "no_eos": (text, dict(temperature=1.0, no_eos=True), dict(plant=[(0, eos, 14.0), (1, eos, 14.0), (2, eos, 14.0)])),
        "finished row": (text, dict(temperature=0.8), dict(done=[0, 1, 0])),
    }


_BASE = {}


def _case(V, ld, B, name, seed):
    """-> logits bf16-valued f32 [B, ld], noise f32 [B, V], tokens, n, done, selection arguments"""
    eos, tb = _ids(V)
    gen, kw, edit = _modes(V)[name]
    if (ld, B) not in _BASE:                          # one random draw per shape, shared by the modes
        _BASE[(ld, B)] = torch.randn(B, ld, generator=torch.Generator().manual_seed(ld + B)) * 2.0
    logits = _BASE[(ld, B)].clone()
    if "ts_shift" in edit:
        logits[:, tb:V] += edit["ts_shift"]
    for b, c, v in edit.get("plant", []):
        if b < B:
            logits[b, c] = v
    if edit.get("peak"):                             # a unique maximum per row
        for b in range(B):
            logits[b, 500 + 7 * b] = 15.0
    logits = logits.bfloat16().float().numpy()
    tokens = np.zeros((B, LD_TOK), dtype=np.int64)
    for b in range(B):
        row = [eos + 1, eos + 2, eos + 7, 50] + list(gen[b])
        tokens[b, :len(row)] = row
    n = P + len(gen[0])
    done = np.array(edit.get("done", [0, 0, 0])[:B] if B > 1 else [int("done" in edit)], dtype=bool)
    full = dict(suppress=None, begin_suppress=None, first=n == P, no_eos=False, ts_begin=-1, max_initial=-1, begin_index=P, eos=eos,
                fill=eos, repetition_penalty=1.0, no_repeat_ngram=0, temperature=1.0, top_k=0, top_p=1.0)
    full.update(kw)
    return logits, sr.exponential_noise((B, V), seed), tokens, n, done, full


def _launch(ops, logits, noise, V, tokens, n, done, kw):
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()       # noqa: E731
    dl, dn, dt, dd = dev(logits).bfloat16(), dev(noise), dev(tokens), dev(done)
    cur = torch.full((tokens.shape[0], 1), -7, dtype=torch.int64, device="cuda")
    dkw = {k: (dev(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    ops.sample_select(dl, V, dt, n, cur, dn, done=dd, **dkw)
    torch.cuda.synchronize()
    return dt.cpu().numpy(), dd.cpu().numpy(), cur.cpu().numpy()


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("V,ld", SHAPES)
def test_kernel_against_the_restatement(ops, V, ld, B):
    for mi, name in enumerate(_modes(V)):
        logits, noise, tokens, n, done, kw = _case(V, ld, B, name, seed=1000 * mi + V % 1000 + B)
        want, want_done, margins = sr.sample_select_ref(logits, noise, V, tokens, n, done=done, **kw)
        what = (name, {k: [f"{x:.3g}" for x in v] for k, v in margins.items()})
        assert not (sr.near(margins) & ~done).any(), what                   # (decided here, before the kernel runs)
        got_tok, got_done, cur = _launch(ops, logits, noise, V, tokens, n, done, kw)
        assert got_tok[:, n].tolist() == want.tolist(), what
        assert cur[:, 0].tolist() == want.tolist(), what
        assert got_done.tolist() == want_done.tolist(), what
        assert np.array_equal(got_tok[:, :n], tokens[:, :n]) and np.array_equal(got_tok[:, n + 1:], tokens[:, n + 1:])
        # the same launch twice gives identical output
        again = _launch(ops, logits, noise, V, tokens, n, done, kw)
        assert np.array_equal(again[0], got_tok) and np.array_equal(again[1], got_done) and np.array_equal(again[2], cur), name
        eos, tb = _ids(V)
        live = [int(t) for t, d in zip(want, done) if not d]
        if name == "top_k=1":
            # whatever the noise: the token of the greedy kernel under the same rules (rows with a unique maximum)
            dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()   # noqa: E731
            dt, cur2 = dev(tokens), torch.zeros(B, 1, dtype=torch.int64, device="cuda")
            ops.greedy_select_history(dev(logits).bfloat16(), V, dt, n, cur2, first=n == P, begin_index=P, eos=eos, fill=eos,
                                      done=dev(done), repetition_penalty=1.0, no_repeat_ngram=0)
            assert cur2[:, 0].tolist() == want.tolist() == [500 + 7 * b for b in range(B)]
        if name in ("timestamps: first token", "timestamps: mass rule fires"):
            assert all(t >= tb for t in live), name
        if name in ("timestamps: closed pair", "timestamps: mass rule quiet"):
            assert all(t < tb for t in live), name
        if name == "timestamps: text + timestamp":
            assert all(t >= tb or t == eos for t in live), name
        if name == "no_eos":
            assert eos not in live
        if name == "first, begin-suppress":
            assert eos not in live and 220 not in live
        if name == "finished row":
            assert all(int(want[b]) == eos for b in range(B) if done[b]) and done.any()


def test_fixture_scenarios_through_the_kernel(ops):
    from test_sample_select import inputs
    for sc in GOLD["scenarios"]:
        logits, noise, tokens, done, kw = inputs(sc)
        B, V = sc["B"], sc["V"]
        padded = np.zeros((B, (V + 3) // 4 * 4), dtype=np.float32)
        padded[:, :V] = logits
        got_tok, got_done, cur = _launch(ops, padded, noise, V, tokens, sc["n"], done, kw)
        assert got_tok[:, sc["n"]].tolist() == sc["expected"], sc["name"]
        assert cur[:, 0].tolist() == sc["expected"] and got_done.astype(int).tolist() == sc["expected_done"], sc["name"]


# ---- decoder and generate: kernel (graphs on / off) against the torch path under one seed -------------------------------------
ARGS = [dict(temperature=0.8), dict(temperature=1.3, top_k=5), dict(temperature=0.7, top_p=0.6, repetition_penalty=1.2)]
SCEN = dict(seed=11, ts_fields=False, B=2, kind="short")


def _decoder_run(ops, monkeypatch, soft, *, graphs, torch_path, seed, max_new=20):
    from distil_whisper_amd import decoding
    monkeypatch.setenv(decoding.SAMPLE_TORCH_ENV, "1" if torch_path else "0")
    model = hr.dropin(ops, SCEN)
    eng = model.engine
    enc, _ = eng.encode(hr.inputs_of(SCEN).cuda().to(torch.float32).contiguous(), save=False)
    prompt = torch.tensor([[gd.SOT, gd.LANG["<|en|>"], gd.TRANSCRIBE, gd.NOTIMESTAMPS]] * SCEN["B"], device="cuda")
    dec = decoding.GreedyDecoder(eng, SCEN["B"], prompt.shape[1] + max_new, eos_token_id=gd.EOS,
                                 suppress_tokens=gd.SUPPRESS + list(range(gd.TS0, gd.V)), begin_suppress_tokens=gd.BEGIN_SUPPRESS,
                                 use_graphs=graphs, pad_token_id=gd.EOS, soft=dict(soft, do_sample=True))
    assert (dec.sample is None) == torch_path and dec.use_graphs == (graphs and not torch_path)
    torch.manual_seed(seed)
    out = dec.run(enc, prompt, max_new).tolist()
    if graphs and not torch_path:
        assert len(dec.graphs) > 0                    # the sampled steps really were replayed from HIP graphs
    return out, torch.cuda.get_rng_state()


@pytest.mark.parametrize("args", ARGS, ids=lambda a: ",".join(f"{k}={v}" for k, v in a.items()))
def test_decoder_kernel_with_and_without_graphs_equals_the_torch_path(ops, monkeypatch, args):
    soft = dict(temperature=args.get("temperature"), top_k=args.get("top_k"), top_p=args.get("top_p"),
                repetition_penalty=args.get("repetition_penalty"), no_repeat_ngram_size=0)
    runs = {k: _decoder_run(ops, monkeypatch, soft, graphs=g, torch_path=t, seed=1234)
            for k, (g, t) in dict(graphs=(True, False), eager=(False, False), torch=(True, True)).items()}
    assert runs["graphs"][0] == runs["torch"][0] and runs["eager"][0] == runs["torch"][0]
    assert torch.equal(runs["graphs"][1], runs["torch"][1]) and torch.equal(runs["eager"][1], runs["torch"][1])
    other, _ = _decoder_run(ops, monkeypatch, soft, graphs=True, torch_path=False, seed=4321)
    ref = runs["torch"][0]
    assert [len(r) for r in other] == [len(r) for r in ref] and other != ref
    banned = set(gd.SUPPRESS) | set(range(gd.TS0, gd.V))
    for row in other:
        assert all(0 <= t < gd.V for t in row) and not (set(row[4:]) - {gd.EOS}) & banned


def _generate(ops, monkeypatch, torch_path, seed, **kw):
    from distil_whisper_amd import decoding
    monkeypatch.setenv(decoding.SAMPLE_TORCH_ENV, "1" if torch_path else "0")
    sc = dict(SCEN, ts_fields=True, frames=450) if kw.get("return_timestamps") else SCEN     # (a short window: a quick seek loop)
    model = hr.dropin(ops, sc)
    f = hr.inputs_of(sc).cuda()
    torch.manual_seed(seed)
    out = model.generate(f, language="en", **kw).tolist()
    return out, model


@pytest.mark.parametrize("args", ARGS, ids=lambda a: ",".join(f"{k}={v}" for k, v in a.items()))
def test_generate_kernel_equals_the_torch_path(ops, monkeypatch, args):
    got, model = _generate(ops, monkeypatch, False, 77, max_new_tokens=12, use_graphs=True, **args)
    (dec,) = model._decoders.values()
    assert dec.sample is not None and dec.use_graphs and len(dec.graphs) > 0
    want, model = _generate(ops, monkeypatch, True, 77, max_new_tokens=12, use_graphs=True, **args)
    (dec,) = model._decoders.values()
    assert dec.sample is None and not dec.use_graphs
    assert got == want


def test_generate_fallback_passes_sample_in_the_kernel(ops, monkeypatch):
    kw = dict(temperature=(0.0, 0.5), compression_ratio_threshold=0.5, logprob_threshold=-1.0, return_timestamps=True,
              max_new_tokens=8)
    calls = []
    real = type(ops).sample_select
    monkeypatch.setattr(type(ops), "sample_select", lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    a, _ = _generate(ops, monkeypatch, False, 5, **kw)
    assert calls                                      # the thresholds sent rows into the sampled pass, and it took the kernel
    n_kernel = len(calls)
    b, _ = _generate(ops, monkeypatch, False, 5, **kw)
    assert a == b
    calls.clear()
    c, _ = _generate(ops, monkeypatch, True, 5, **kw)
    assert not calls and n_kernel > 0
    assert a == c
