"""Scores of finished sequences on the MI355X: the scoring kernel (csrc/score.hip) against its float64 restatement
(tests/score_restatement.py) on random logits, against the token-selection kernel of the decoding loop (csrc/decode.hip), and
`generate(output_scores=True, output_logits=True, return_dict_in_generate=True)` end to end on tests/golden/generate_scores.npz.

Where the bounds come from:
  * `scores` and `chosen`: none.  A kept column is the logit widened to fp32 (exact), a masked one is -inf; which columns are
    masked depends on the logits only through the timestamp mass rule, and rows whose decision lies within 1e-3 of its
    threshold are redrawn (none is skipped);
  * `logprob`: 1e-4 absolute.  A tree sum of at most 54 k fp32 terms with a fast exp and log stays below about 1e-5; a wrong mask
    moves it by far more;
  * end to end: tokens equal, `-inf` pattern identical, finite values within 2 x `ref_bf16_dev` of the fp32 reference (two
    independent bf16 roundings of the same fp32 value differ by at most their sum), HIP graphs on and off bit-identical."""
import numpy as np
import pytest
import torch

import score_restatement as sr

pytestmark = pytest.mark.gpu

META, ARR = sr.gold()
SC = {s["name"]: s for s in META["scenarios"]}
B, L, P = 3, 6, 4
# V, ld: the micro vocabulary (one chunk, ld == V), Whisper's (the register path, ld > V, V % 4 != 0), and one beyond
# 13 x 4096 columns (the loop path)
SHAPES = [(1000, 1000), (51866, 51904), (53302, 53312)]


@pytest.fixture(scope="module")
def ops():
    from distil_whisper_amd.ops_hip import HipOps
    return HipOps("cuda:0")


def _ids(V):
    eos = V - 100
    return eos, V - 88                              # eos, first timestamp id (<|notimestamps|> = tb - 1)


def _tokens(V):
    """Histories that reach every branch of the rules (generated part, L = 6 per row; `t` text, `s` timestamp):
    row 0  s t t s s t   first position; after one timestamp (text only); timestamps not below the last; text + timestamp
                          (timestamp or EOS, the same value may close the pair); a closed pair (text only)
    row 1  t t s E p p   no timestamp yet; text + timestamp; a row that has finished and is padded
    row 2  s s t s t t   a closed pair right at the start; text + timestamp later on; text after it"""
    eos, tb = _ids(V)
    gen = [[tb + 5, 41, 500, tb + 20, tb + 20, 77],
           [42, 600, tb + 9, eos, eos, eos],
           [tb + 0, tb + 3, 43, tb + 30, 44, 45]]
    prompt = [[eos + 1, eos + 2, eos + 7, 50]] * B
    return torch.tensor([p + g for p, g in zip(prompt, gen)], dtype=torch.int64)


def _masks(V):
    eos, tb = _ids(V)
    sup = torch.zeros(V, dtype=torch.uint8)
    sup[:40] = 1
    sup[300:340] = 1
    sup[eos + 1:tb - 1] = 1
    sup[tb + 50] = 1                               # a suppressed timestamp
    sup[77] = 1                                    # a token the sequences hold: its `chosen` is -inf
    bsup = torch.zeros(V, dtype=torch.uint8)
    bsup[[220, eos, tb + 1]] = 1
    return sup, bsup


def _configs(V):
    eos, tb = _ids(V)
    sup, bsup = _masks(V)
    return {
        "timestamps, max_initial, masks, min_new": dict(suppress=sup, begin_suppress=bsup, min_new=4, ts_begin=tb, max_initial=50, eos=eos),
        "timestamps, no max_initial, no masks": dict(ts_begin=tb, max_initial=-1, eos=eos),
        "masks and min_new without timestamp rules": dict(suppress=sup, begin_suppress=bsup, min_new=3, eos=eos),
        "raw": dict(),
    }


def _row(V, ld, seed):
    """one row of logits: sigma 1.5, the timestamp columns shifted as a block so that the mass rule falls either way"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(ld, generator=g) * 1.5
    _, tb = _ids(V)
    x[tb:V] += (torch.rand(1, generator=g).item() - 0.5) * 6.0
    return x


def _draw(V, ld, dtype, tokens, seed0):
    """logits [B * L, ld] whose every mass-rule decision (of every configuration) keeps 1e-3 from its threshold: a row that
    does not is redrawn from the next seed"""
    seeds = [[seed0 + 100 * (b * L + j) for j in range(L)] for b in range(B)]
    logits = torch.stack([_row(V, ld, seeds[b][j]) for b in range(B) for j in range(L)]).to(dtype)
    cfgs = _configs(V)
    for _ in range(20):
        refs = {k: sr.score_tokens_ref(logits, V, tokens, P, L, **kw) for k, kw in cfgs.items()}
        close = {(b, j) for r in refs.values() for b in range(B) for j in range(L)
                 if r[3][b][j] is not None and r[3][b][j] < 1e-3}
        if not close:
            return logits, refs
        for b, j in close:
            seeds[b][j] += 1
            logits[b * L + j] = _row(V, ld, seeds[b][j]).to(dtype)
    raise AssertionError("rows still within 1e-3 of the mass-rule threshold after 20 redraws")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("V,ld", SHAPES)
def test_score_tokens_against_the_float64_restatement(ops, V, ld, dtype):
    tokens = _tokens(V)
    logits, refs = _draw(V, ld, dtype, tokens, seed0=7 * V)
    dl, dt = logits.cuda(), tokens.cuda()
    decisions = set()
    for name, kw in _configs(V).items():
        dkw = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in kw.items()}
        sc, chosen, logprob = ops.score_tokens(dl, V, dt, P, L, **dkw)
        torch.cuda.synchronize()
        want_sc, want_chosen, want_lp, margins = refs[name]
        assert sc.shape == (L, B, V) and chosen.shape == (B, L) and logprob.shape == (B, L)
        sc, chosen, logprob = sc.cpu(), chosen.cpu(), logprob.cpu()
        assert torch.equal(torch.isneginf(sc), torch.isneginf(want_sc)), name
        assert torch.equal(sc.view(torch.int32), want_sc.view(torch.int32)), name       # bit for bit
        assert torch.equal(chosen.view(torch.int32), want_chosen.view(torch.int32)), name
        assert torch.equal(torch.isneginf(logprob), torch.isneginf(want_lp)), name
        fin = torch.isfinite(want_lp)
        dev = (logprob[fin] - want_lp[fin]).abs().max().item()
        print(f"V={V} {dtype} [{name}]: logprob max abs dev {dev:.2e}; masked chosen {int(torch.isneginf(want_chosen).sum())}")
        assert dev <= 1e-4, name
        if name == "raw":
            assert torch.equal(sc, logits[:, :V].float().view(B, L, V).transpose(0, 1))
            assert torch.isfinite(logprob).all()
        else:
            assert torch.isneginf(want_chosen).any()                # the sequences hold tokens the rules mask
        if "ts_begin" in kw:
            _, tb = _ids(V)
            decisions |= {bool(torch.isneginf(want_sc[j, b, :tb]).all()) for b in range(B) for j in range(1, L)
                          if margins[b][j] is not None}
        # scores alone / chosen alone give the same values
        only_sc, c2, l2 = ops.score_tokens(dl, V, dt, P, L, want_chosen=False, **dkw)
        assert c2 is None and l2 is None and torch.equal(only_sc.cpu().view(torch.int32), sc.view(torch.int32))
        s3, only_c, only_l = ops.score_tokens(dl, V, dt, P, L, want_scores=False, **dkw)
        assert s3 is None and torch.equal(only_c.cpu().view(torch.int32), chosen.view(torch.int32))
        assert torch.equal(only_l.cpu().view(torch.int32), logprob.view(torch.int32))
    assert decisions == {True, False}                               # the mass rule fell both ways


def test_batch_pitch_and_token_pitch(ops):
    """rows of a longer pass (batch_rows > L, the view generate hands over) and a token buffer wider than prompt + steps"""
    V, ld = 1000, 1024
    tokens = _tokens(V)
    logits, refs = _draw(V, ld, torch.bfloat16, tokens, seed0=99)
    name, kw = next(iter(_configs(V).items()))
    rows = L + 5
    big = torch.full((B * rows + 3, ld), 7.0, dtype=torch.bfloat16)
    for b in range(B):
        big[3 + b * rows:3 + b * rows + L] = logits[b * L:(b + 1) * L]
    wide = torch.cat([tokens, torch.full((B, 7), 5, dtype=torch.int64)], 1)
    dkw = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in kw.items()}
    sc, chosen, logprob = ops.score_tokens(big.cuda()[3:], V, wide.cuda(), P, L, batch_rows=rows, **dkw)
    torch.cuda.synchronize()
    assert torch.equal(sc.cpu().view(torch.int32), refs[name][0].view(torch.int32))
    assert torch.equal(chosen.cpu().view(torch.int32), refs[name][1].view(torch.int32))


@pytest.mark.parametrize("V,ld", SHAPES)
def test_argmax_of_the_scores_is_the_token_greedy_select_picks(ops, V, ld):
    """the two kernels that hold the rules (csrc/decode.hip during decoding, csrc/score.hip afterwards) against each other:
    the smallest index among the maxima of each processed row is the token the selection kernel writes"""
    tokens = _tokens(V)
    logits, _ = _draw(V, ld, torch.bfloat16, tokens, seed0=7 * V)
    dl, dt = logits.cuda(), tokens.cuda()
    eos, tb = _ids(V)
    for name, kw in _configs(V).items():
        dkw = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in kw.items()}
        sc, _, _ = ops.score_tokens(dl, V, dt, P, L, **dkw)
        want = sc.argmax(-1)                                       # [L, B] (torch: the first of equal maxima)
        mx = sc.max(-1, keepdim=True).values
        first = torch.where(sc == mx, torch.arange(V, device="cuda")[None, None, :], V).min(-1).values
        assert torch.equal(first, want)
        for j in range(L):
            hist = dt.clone()
            cur = torch.zeros(B, 1, dtype=torch.int64, device="cuda")
            done = torch.zeros(B, dtype=torch.bool, device="cuda")
            ops.greedy_select(dl.view(B, L, ld)[:, j], V, hist, P + j, cur, suppress=dkw.get("suppress"),
                              begin_suppress=dkw.get("begin_suppress"), first=j == 0, no_eos=j < kw.get("min_new", 0),
                              ts_begin=kw.get("ts_begin", -1), max_initial=kw.get("max_initial", -1), begin_index=P,
                              eos=kw.get("eos", -1), fill=eos, done=done)
            assert cur[:, 0].tolist() == want[j].tolist(), (name, j)


@pytest.mark.parametrize("name", ["plain", "min_new_tokens", "prompt_ids", "timestamps", "ragged_finish"])
def test_generate_end_to_end(ops, name):
    sc = SC[name]
    model = sr.dropin(ops, sc)
    outs = {}
    for graphs in (False, True):
        _, out = sr.run_dropin(ops, sc, model=model, use_graphs=graphs)
        assert out.scores is not None and out.logits is not None
        assert out.sequences.tolist() == ARR[f"{name}.sequences"].tolist(), f"graphs={graphs}"
        assert len(out.scores) == len(out.logits) == sc["steps"]
        outs[graphs] = out
        bound = 2 * sc["ref_bf16_dev"]
        for field in ("scores", "logits"):
            got, want = sr.stacked(out[field]), ARR[f"{name}.{field}"]
            assert np.array_equal(np.isneginf(got), np.isneginf(want)), f"{name}.{field}: other columns are masked"
            fin = np.isfinite(want)
            dev = float(np.abs(got[fin] - want[fin]).max())
            print(f"{name}.{field} graphs={graphs}: max |ours - fp32 reference| {dev:.4f} (bound {bound:.4f})")
            assert dev <= bound
        # the kernel's per-token values are the gather over its own tensors; a kept score is the raw logit
        st = torch.stack(tuple(out.scores), 1)
        idx = out.sequences[:, sc["P"]:, None]
        assert torch.equal(model.compute_transition_scores(out.sequences, out.scores), st.gather(2, idx)[:, :, 0])
        lp = model.compute_transition_scores(out.sequences, out.scores, normalize_logits=True)
        ref_lp = torch.log_softmax(st, -1).gather(2, idx)[:, :, 0]
        assert torch.equal(torch.isneginf(lp), torch.isneginf(ref_lp))
        assert (lp - ref_lp)[torch.isfinite(ref_lp)].abs().max().item() <= 1e-4
        raw = torch.stack(tuple(out.logits), 1)
        assert torch.equal(st[torch.isfinite(st)], raw[torch.isfinite(st)])
    for field in ("scores", "logits"):
        assert all(torch.equal(a, b) for a, b in zip(outs[False][field], outs[True][field])), f"{field}: graphs change the values"
