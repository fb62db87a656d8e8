"""`sequence_bias` / `bad_words_ids` inside the selection kernel on the MI355X (`dw_greedy_select_bias`, csrc/decode.hip): the kernel
against its float64 restatement (tests/sequence_bias_restatement.py) on planted rows, against `dw_greedy_select_history` without a
table, and the decoder / `generate` end to end on the micro model and on tests/golden/sequence_bias.json with HIP graphs off and on.

Where the bounds come from: none is needed.  Every row is a background far below (-30 .. -22) plus a handful of planted logits,
the planted logits and the biases are multiples of 0.25 with few significant bits, so every biased value x + bias is exact in fp32
and in float64 alike; the penalised value is one IEEE multiply or divide of that.  Every decision -- the top two processed values of a
row, and the timestamp mass rule against its threshold -- is planted at least 0.25 apart (`_expect` asserts it on the restatement
before anything is launched), against differences of the order 1e-6 between the kernel's fp32 / fast-exponential arithmetic and
float64.  Tokens, `done` and `cur` must be equal."""
import numpy as np
import pytest
import torch

import beam_cases as bc
import sequence_bias_restatement as br
from oracle import gen_golden_decode as gd

pytestmark = pytest.mark.gpu

GOLD = br.gold()
SC = {s["name"]: s for s in GOLD["scenarios"]}
B, P, LD_TOK = 3, 4, 16
# V, ld: one chunk row whose last chunk of four columns is partial; Whisper's two vocabularies (the register path, ld > V); one
# beyond 13 x 4096 columns (the loop path, ld == V)
SHAPES = [(1030, 1032), (51865, 51872), (51866, 51904), (53252, 53252)]
A_, B_, C_, D_, FREE = 101, 202, 405, 640, 500   # text ids that are planted
X, Y, Z, JUNK = 61, 62, 63, 77                   # text ids the histories hold; what the token buffer holds beyond position n
MIN_GAP = 0.25


@pytest.fixture(scope="module")
def ops():
    from distil_whisper_amd.ops_hip import HipOps
    return HipOps("cuda:0")


def _ids(V):
    return V - 100, V - 88                          # eos, first timestamp id (<|notimestamps|> = tb - 1)


def _prompt(V):
    eos, _ = _ids(V)
    return [eos + 1, eos + 2, eos + 7, 50]


def _configs(V):
    eos, tb = _ids(V)
    sup = torch.zeros(V, dtype=torch.uint8)
    sup[:40] = 1
    sup[300:340] = 1
    sup[eos + 1:tb - 1] = 1
    bsup = torch.zeros(V, dtype=torch.uint8)
    bsup[[220, eos, tb + 1]] = 1
    return {"plain": dict(eos=eos), "masks": dict(suppress=sup, begin_suppress=bsup, eos=eos),
            "timestamps": dict(ts_begin=tb, max_initial=-1, eos=eos),
            "timestamps, masks": dict(suppress=sup, begin_suppress=bsup, ts_begin=tb, max_initial=50, eos=eos)}


def _cases(V):
    """gen: the generated part of each row's history (behind the prompt); plant: (row, column, logit); sb / bw: the arguments;
    picks: the token each row must take (asserted on the restatement); off: rows whose token must differ without the table."""
    eos, tb = _ids(V)
    rng = np.random.default_rng(V)
    lay = dict(tb=tb, eos=eos)
    hist0 = _prompt(V) + [X, Y, Z]
    ts_table = dict(sb=[[[tb + 9], 1.5], [[A_], 1.0]], bw=[[tb + 12]])
    return {
        # a boost lifts the third best to the top (row 0), a negative bias drops the raw best (row 1), row 2 holds no biased id
        "boost and drop": dict(gen=[[X, Y, Z]] * 3, sb=[[[C_], 1.5], [[A_], -1.0]],
                               plant=[(0, A_, 12.0), (0, B_, 11.5), (0, C_, 11.0), (1, A_, 12.0), (1, B_, 11.5), (2, D_, 12.0), (2, FREE, 11.0)],
                               picks=[C_, B_, D_], off=[0, 1]),
        "prefix in row 0 only": dict(gen=[[Z, X, Y], [Z, Y, X], [X, Z, Y]], sb=[[[X, Y, C_], 2.0]],
                                     plant=[(b, c, v) for b in range(3) for c, v in ((A_, 12.0), (C_, 10.5))],
                                     picks=[C_, A_, A_], off=[0]),
        # n = 7: a sequence of n tokens applies (its prefix is the history without its first token), one of n + 1 tokens is
        # ignored although the whole history is its prefix (applied, it would win)
        "length rule": dict(gen=[[X, Y, Z], [X, Y, Y], [Y, Y, Z]], sb=[[hist0[1:] + [C_], 2.0], [hist0 + [D_], 2.0]],
                            plant=[(b, c, v) for b in range(3) for c, v in ((A_, 12.0), (C_, 10.5), (D_, 11.75))],
                            picks=[C_, A_, A_], off=[0]),
        "prefix straddles the prompt": dict(gen=[[X], [Y], [X]], sb=[[[eos + 7, 50, X, C_], 2.0]],
                                            plant=[(b, c, v) for b in range(3) for c, v in ((A_, 12.0), (C_, 10.5))],
                                            picks=[C_, A_, C_], off=[0, 2]),
        # the buffer holds JUNK from position n on: a kernel that read one token too far would meet these prefixes
        "pad beyond n": dict(gen=[[X, Y, Z]] * 3, sb=[[[JUNK, C_], 2.0], [[Z, JUNK, C_], 2.0]],
                             plant=[(b, c, v) for b in range(3) for c, v in ((A_, 12.0), (C_, 10.5))], picks=[A_, A_, A_], off=[]),
        # row 0: two sequences and the one-token entry meet on one column (10.5 + 0.75 + 0.75 + 0.25 > 12); row 1: one of them
        "two hits on one column": dict(gen=[[Z, Y, X], [Z, Z, X], [Z, Y, Y]], sb=[[[X, C_], 0.75], [[Y, X, C_], 0.75], [[C_], 0.25]],
                                       plant=[(b, c, v) for b in range(3) for c, v in ((A_, 12.0), (C_, 10.5))],
                                       picks=[C_, A_, A_], off=[0]),
        "bad words": dict(gen=[[Z, Y, X], [Z, Y, Y], [Z, Y, X]], bw=[[X, A_], [D_], [eos]],
                          plant=[(0, A_, 12.0), (0, B_, 11.0), (1, A_, 12.0), (1, B_, 11.0), (2, D_, 12.0), (2, A_, 11.5), (2, B_, 11.0)],
                          picks=[B_, A_, B_], off=[0, 2]),
        # [eos] alone is dropped on the host: EOS is still taken (row 0), also when a bad word removes the raw best (row 1)
        "eos entry filtered": dict(gen=[[X, Y, Z]] * 3, bw=[[eos], [D_]],
                                   plant=[(0, eos, 12.0), (0, A_, 11.0), (1, D_, 12.0), (1, eos, 11.5), (1, A_, 11.0), (2, A_, 12.0)],
                                   picks=[eos, eos, A_], off=[1]),
        # the bias comes BEFORE the penalty: (8 + 4) / 1.5 = 8 < 8.75, the other order would give 9.33; row 2: (-10 + 4) * 1.5 = -9
        "biased and seen, penalty 1.5": dict(gen=[[A_, Y, Z]] * 3, sb=[[[A_], 4.0]], penalty=1.5,
                                             plant=[(0, A_, 8.0), (0, FREE, 8.75), (1, A_, 8.0), (1, FREE, 7.0), (2, A_, -10.0),
                                                    (2, FREE, -10.0)], picks=[FREE, A_, A_], off=[1, 2]),
        # (8 + 4) / 0.8 = 15 > 14.5, the other order would give 14
        "biased and seen, penalty 0.8": dict(gen=[[A_, Y, Z]] * 3, sb=[[[A_], 4.0]], penalty=0.8,
                                             plant=[(0, A_, 8.0), (0, FREE, 14.5), (1, A_, 8.0), (1, FREE, 16.0), (2, A_, -10.0),
                                                    (2, FREE, -5.5)], picks=[A_, FREE, A_], off=[0, 2]),
        "biased and suppressed": dict(gen=[[X, Y, Z]] * 3, sb=[[[310], 8.0], [[A_], 0.5]], cfg="masks",
                                      plant=[(b, c, v) for b in range(3) for c, v in ((310, 12.0), (A_, 11.0), (B_, 11.25))],
                                      picks=[A_, A_, A_], off=[0, 1, 2]),
        # with both history rules: row 0 -- Y is boosted but completes a 2-gram, the prefix (X) boosts A; row 1 -- Y is boosted,
        # then penalised: (9 + 3) / 1.25 = 9.6 < 10.5; row 2 -- X completes a 2-gram
        "with the history rules": dict(gen=[[X, Y, X], [X, Y, Z], [Y, X, Y]], sb=[[[Y], 3.0], [[X, A_], 1.0]], penalty=1.25, ngram=2,
                                       plant=[(0, Y, 12.0), (0, A_, 10.0), (0, B_, 10.5), (1, Y, 9.0), (1, B_, 10.5), (2, X, 12.0),
                                              (2, A_, 10.0)], picks=[A_, B_, A_], off=[0]),
        # ---- the timestamp rules, every state of tests/beam_cases.history ----
        # row 0: the boost of one timestamp turns the mass rule (logsumexp(9, 9) = 9.69 < 10 < 10.31 = logsumexp(10, 9))
        "mass rule flips": dict(gen=[bc.history("open", lay, rng, 3)] * 3, sb=[[[tb + 10], 1.0]], cfg="timestamps",
                                plant=[(0, A_, 10.0), (0, tb + 10, 9.0), (0, tb + 11, 9.0), (1, A_, 10.0), (1, tb + 10, 7.0),
                                       (1, tb + 11, 7.0), (2, A_, 8.0), (2, tb + 10, 9.0)],
                                picks=[tb + 10, A_, tb + 10], off=[0], flips=[0]),
        "state text": dict(gen=[[X, Y, Z]] * 3, cfg="timestamps", **ts_table,
                           plant=[(0, A_, 10.0), (0, B_, 10.5), (0, tb + 12, 12.0), (0, tb + 9, 8.0), (1, A_, 9.0), (1, B_, 10.5),
                                  (2, tb + 9, 11.0), (2, A_, 10.0)], picks=[A_, B_, tb + 9], off=[0], flips=[0]),
        "state open": dict(gen=[bc.history("open", lay, rng, 3)] * 3, cfg="timestamps", **ts_table,
                           plant=[(0, A_, 10.0), (0, B_, 10.5), (0, tb + 12, 12.0), (0, tb + 9, 8.0), (1, tb + 12, 12.0), (1, B_, 10.5),
                                  (2, tb + 9, 10.0), (2, B_, 10.5)], picks=[A_, B_, tb + 9], off=[0, 1, 2], flips=[0, 1, 2]),
        "state text_ts": dict(gen=[bc.history("text_ts", lay, rng, 3)] * 3, cfg="timestamps", **ts_table,
                              plant=[(0, eos, 9.0), (0, tb + 9, 8.0), (0, tb + 12, 12.0), (0, A_, 13.0), (1, eos, 10.0), (1, tb + 9, 8.0),
                                     (2, tb + 20, 10.0), (2, tb + 9, 8.0)], picks=[tb + 9, eos, tb + 20], off=[0]),
        "state pair": dict(gen=[bc.history("pair", lay, rng, 3)] * 3, cfg="timestamps", **ts_table,
                           plant=[(0, A_, 10.0), (0, B_, 10.5), (0, tb + 9, 14.0), (1, A_, 9.0), (1, B_, 10.5), (2, tb + 9, 14.0),
                                  (2, C_, 5.0)], picks=[A_, B_, C_], off=[0]),
        "first step": dict(gen=[[]] * 3, cfg="timestamps, masks", **ts_table,
                           plant=[(0, tb + 9, 8.0), (0, tb + 12, 12.0), (0, tb + 3, 9.0), (0, A_, 15.0), (1, tb + 3, 10.0),
                                  (1, tb + 9, 8.0), (2, tb + 60, 15.0), (2, tb + 9, 8.0)], picks=[tb + 9, tb + 3, tb + 9], off=[0]),
    }


def _inputs(V, ld, case, seed):
    g = torch.Generator().manual_seed(seed)
    logits = torch.rand(B, ld, generator=g) * 8.0 - 30.0
    for b, c, v in case["plant"]:
        logits[b, c] = v
    tokens = torch.full((B, LD_TOK), JUNK, dtype=torch.int64)
    for b in range(B):
        row = _prompt(V) + list(case["gen"][b])
        tokens[b, :len(row)] = torch.tensor(row)
    n = P + len(case["gen"][0])
    done = torch.zeros(B, dtype=torch.bool)
    kw = _configs(V)[case.get("cfg", "plain")]
    eos, _ = _ids(V)
    skw = dict(suppress=kw.get("suppress"), begin_suppress=kw.get("begin_suppress"), first=n == P, no_eos=False,
               ts_begin=kw.get("ts_begin", -1), max_initial=kw.get("max_initial", -1), begin_index=P, eos=kw["eos"], fill=eos)
    return logits.bfloat16(), tokens, n, done, skw


def _expect(V, case, logits, tokens, n, done, skw):
    """the restatement's answer, with the design of the case asserted on it: the picks, the gap of every decision, the rows the
    table changes, the rows whose mass rule it turns"""
    opts = dict(repetition_penalty=case.get("penalty", 1.0), no_repeat_ngram=case.get("ngram", 0))
    want, want_done, margins, sides = br.select_bias_ref(logits, V, tokens, n, sequence_bias=case.get("sb"),
                                                         bad_words_ids=case.get("bw"), done=done, **skw, **opts)
    assert want.tolist() == case["picks"], (want.tolist(), case["picks"])
    assert min(margins) >= MIN_GAP, margins
    off, _, off_margins, off_sides = br.select_bias_ref(logits, V, tokens, n, done=done, **skw, **opts)
    assert min(off_margins) >= MIN_GAP, off_margins
    assert [b for b in range(B) if int(off[b]) != int(want[b])] == case["off"]
    assert [b for b in range(B) if sides[b] is not None and sides[b] != off_sides[b]] == case.get("flips", [])
    return want, want_done, off


def _table(case, V, device):
    from distil_whisper_amd.decoding import sequence_bias_table
    table = sequence_bias_table(case.get("sb"), case.get("bw"), V, _ids(V)[0])
    return {} if table is None else table.tensors(device)


def _launch(fn, logits, V, tokens, n, done, skw, **opts):
    dl, dt, dd = logits.cuda(), tokens.cuda(), done.cuda()
    cur = torch.full((B, 1), -7, dtype=torch.int64, device="cuda")
    dkw = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in skw.items()}
    fn(dl, V, dt, n, cur, done=dd, **dkw, **opts)
    torch.cuda.synchronize()
    return dt.cpu(), dd.cpu(), cur.cpu()


@pytest.mark.parametrize("V,ld", SHAPES)
def test_kernel_against_the_restatement(ops, V, ld):
    for ci, (cname, case) in enumerate(_cases(V).items()):
        logits, tokens, n, done, skw = _inputs(V, ld, case, seed=V + ci)
        want, want_done, _ = _expect(V, case, logits, tokens, n, done, skw)
        got_tok, got_done, cur = _launch(ops.greedy_select_bias, logits, V, tokens, n, done, skw,
                                         repetition_penalty=case.get("penalty", 1.0), no_repeat_ngram=case.get("ngram", 0),
                                         **_table(case, V, "cuda"))
        assert got_tok[:, n].tolist() == want.tolist(), cname
        assert cur[:, 0].tolist() == want.tolist(), cname
        assert got_done.tolist() == want_done.tolist(), cname
        assert torch.equal(got_tok[:, :n], tokens[:, :n]) and torch.equal(got_tok[:, n + 1:], tokens[:, n + 1:]), cname


@pytest.mark.parametrize("V,ld", SHAPES)
def test_without_a_table_it_selects_what_dw_greedy_select_history_selects(ops, V, ld):
    for ci, (cname, case) in enumerate(_cases(V).items()):
        logits, tokens, n, done, skw = _inputs(V, ld, case, seed=V + ci)
        opts = dict(repetition_penalty=case.get("penalty", 1.0), no_repeat_ngram=case.get("ngram", 0))
        a = _launch(ops.greedy_select_history, logits, V, tokens, n, done, skw, **opts)
        b = _launch(ops.greedy_select_bias, logits, V, tokens, n, done, skw, **opts)
        for x, y in zip(a, b):
            assert torch.equal(x, y), cname
    # a forced position copies the prompt token, whatever the table
    tokens = torch.arange(B * LD_TOK, dtype=torch.int64).view(B, LD_TOK).cuda()
    cur = torch.zeros(B, 1, dtype=torch.int64, device="cuda")
    ops.greedy_select_bias(None, V, tokens, 2, cur, forced=True, repetition_penalty=1.7, no_repeat_ngram=2,
                           **_table(dict(sb=[[[5], 1.0]]), V, "cuda"))
    assert cur[:, 0].tolist() == tokens[:, 2].tolist()


def test_a_full_table_of_1024_sequences(ops):
    """every thread tests a sequence: 1024 entries of 1..4 tokens, most of them on shared columns, against the restatement"""
    V, ld = 51866, 51904
    rng = np.random.default_rng(7)
    case = dict(gen=[[X, Y, Z], [Z, Y, X], [Y, Z, X]], plant=[(b, c, v) for b in range(3) for c, v in ((A_, 12.0), (C_, 10.5), (D_, 9.0))])
    sb = {(Y, Z, C_): 2.0}                                    # row 0: lifts C over A whatever else meets that column (|sum| small)
    while len(sb) < 1000:
        q = tuple(int(t) for t in rng.choice([X, Y, Z, 64, 65, 66, 67, 68], size=int(rng.integers(0, 4)))) + (int(rng.choice([A_, C_, D_, FREE, 700, 701])),)
        sb[q] = float(rng.integers(-2, 3)) / 4
    bw = [[int(t), int(c)] for t, c in zip(rng.integers(1000, 2000, 24), rng.integers(2000, 3000, 24))]
    case.update(sb=sb, bw=bw)
    from distil_whisper_amd.decoding import sequence_bias_table
    assert sequence_bias_table(sb, bw, V, _ids(V)[0]).S == 1024
    logits, tokens, n, done, skw = _inputs(V, ld, case, seed=99)
    want, want_done, margins, _ = br.select_bias_ref(logits, V, tokens, n, sequence_bias=sb, bad_words_ids=bw, done=done, **skw)
    assert min(margins) >= MIN_GAP, margins
    got_tok, got_done, cur = _launch(ops.greedy_select_bias, logits, V, tokens, n, done, skw, **_table(case, V, "cuda"))
    assert got_tok[:, n].tolist() == want.tolist() and cur[:, 0].tolist() == want.tolist() and got_done.tolist() == want_done.tolist()


# ---- the decoder and `generate` on the micro model --------------------------------------------------------------------------
def _decode(ops, sc, table, use_graphs, eager=False, **soft):
    from distil_whisper_amd.decoding import GreedyDecoder
    model = br.dropin(ops, sc)
    fields = br.fields_of(sc)
    dec = GreedyDecoder(model.engine, 2, 16, eos_token_id=gd.EOS, suppress_tokens=fields["suppress_tokens"],
                        begin_suppress_tokens=fields["begin_suppress_tokens"], use_graphs=use_graphs,
                        soft=dict(do_sample=False, sequence_bias=table, **soft))
    assert dec.bias is not None and dec.use_graphs == use_graphs
    if eager:                                                 # the torch selection of `_select_soft`, as on ops without the entry
        dec.bias, dec.use_graphs = None, False
    enc, _ = model.engine.encode(br.inputs_of(sc).cuda().float().contiguous(), save=False)
    prompt = torch.tensor([[gd.SOT, 902, gd.TRANSCRIBE, gd.NOTIMESTAMPS]] * 2, device="cuda")
    out = dec.run(enc, prompt, 10).tolist()
    return out, dec


def test_decoder_graphs_equal_no_graphs_equal_the_eager_selection(ops):
    from distil_whisper_amd.decoding import sequence_bias_table
    sc = SC["with_repetition_rules"]
    kw = sc["kwargs"]
    table = sequence_bias_table(kw["sequence_bias"], kw["bad_words_ids"], gd.V, gd.EOS)
    soft = dict(repetition_penalty=kw["repetition_penalty"], no_repeat_ngram_size=kw["no_repeat_ngram_size"])
    plain, _ = _decode(ops, sc, table, False, **soft)
    graphs, dec = _decode(ops, sc, table, True, **soft)
    assert len(dec.graphs) > 0 and graphs == plain
    eager, _ = _decode(ops, sc, table, False, eager=True, **soft)
    assert eager == plain
    assert [row[:len(want)] for row, want in zip(plain, sc["sequences"])] == sc["sequences"]   # (the fixture stops after 8 tokens)


@pytest.mark.parametrize("name", ["one_token_boost", "multi_token_boost", "two_on_one_column", "bad_words", "with_repetition_rules",
                                  "timestamps_one_window"])
def test_generate_end_to_end_with_graphs_off_and_on(ops, name):
    sc = SC[name]
    model = br.dropin(ops, sc)
    for graphs in (False, True):
        assert br.run(model, sc, device="cuda", use_graphs=graphs) == sc["sequences"], f"graphs={graphs}"
        (dec,) = model._decoders.values()
        assert dec.bias is not None and dec.use_graphs == graphs
        if graphs:
            assert len(dec.graphs) > 0                    # the token steps really were replayed from HIP graphs
    # a second call replays the captured graphs on a new history.  (The fixture's `baseline` is not decoded here: the generator
    # checks only the biased output against bf16 and logit noise; tests/test_sequence_bias.py decodes the baseline in fp32.)
    assert br.run(model, sc, device="cuda", use_graphs=True) == sc["sequences"]


def test_seek_loop_end_to_end(ops):
    sc = SC["seek_loop"]
    model = br.dropin(ops, sc)
    assert br.run(model, sc, device="cuda") == sc["sequences"]
    got = model.generate(br.inputs_of(sc).cuda(), return_segments=True, **sc["kwargs"])
    assert [[list(s["tokens"]) for s in row] for row in got["segments"]] == [[s["tokens"] for s in row] for row in sc["segments"]]
    assert all(dec.bias is not None for dec in model._seek_decoders.values()) and model._seek_decoders
