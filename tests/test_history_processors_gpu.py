"""`repetition_penalty` / `no_repeat_ngram_size` inside the selection kernel on the MI355X (`dw_greedy_select_history`,
csrc/decode.hip): the kernel against its restatement (tests/history_restatement.py) on random logits with hand-written histories,
against `dw_greedy_select` with both rules off, and `generate` end to end on tests/golden/history_processors.json with HIP graphs
off and on.

Where the bounds come from: none is needed.  The penalised value is one IEEE fp32 multiply or divide of the widened bf16 logit on
both sides, so the selected token can differ only where two processed values tie (the smallest index wins on both sides) or
where the timestamp mass rule -- a sum of ~90 fast exponentials against a float64 log_softmax -- lies at its threshold: rows whose
top-two distance or mass-rule distance after processing is within 1e-3 are redrawn (none is skipped).  Tokens, `done` and `cur`
must be equal."""
import pytest
import torch

import history_restatement as hr
from oracle import gen_golden_decode as gd

pytestmark = pytest.mark.gpu

GOLD = hr.gold()
SC = {s["name"]: s for s in GOLD["scenarios"]}
B, P, LD_TOK = 3, 4, 16
# V, ld: the micro vocabulary (one chunk, ld == V), Whisper's (the register path, ld > V, V % 4 != 0), and one beyond
# 13 x 4096 columns (the loop path)
SHAPES = [(1000, 1000), (51866, 51904), (53302, 53312)]
A_, B_, C_, FREE = 101, 202, 405, 500              # three text ids the histories hold, one they never hold


@pytest.fixture(scope="module")
def ops():
    from distil_whisper_amd.ops_hip import HipOps
    return HipOps("cuda:0")


def _ids(V):
    return V - 100, V - 88                          # eos, first timestamp id (<|notimestamps|> = tb - 1)


def _masks(V):
    eos, tb = _ids(V)
    sup = torch.zeros(V, dtype=torch.uint8)
    sup[:40] = 1
    sup[300:340] = 1
    sup[eos + 1:tb - 1] = 1
    sup[tb + 50] = 1
    bsup = torch.zeros(V, dtype=torch.uint8)
    bsup[[220, eos, tb + 1]] = 1
    return sup, bsup


def _configs(V):
    eos, tb = _ids(V)
    sup, bsup = _masks(V)
    return {
        "timestamps, masks, min_new": dict(suppress=sup, begin_suppress=bsup, min_new=4, ts_begin=tb, max_initial=50, eos=eos),
        "timestamps": dict(ts_begin=tb, max_initial=-1, eos=eos),
        "masks, min_new": dict(suppress=sup, begin_suppress=bsup, min_new=3, eos=eos),
        "plain": dict(eos=eos),
    }


def _cases(V):
    """Histories (generated part per row; the prompt is [eos+1, eos+2, eos+7, 50]) and planted logits that reach every branch.
    `changed`: (configuration, rows) whose token must differ from what the same inputs give with both rules off."""
    eos, tb = _ids(V)
    return {
        # row 0: a token held twice is penalised ONCE (16 / 2 = 8 stays above 7; twice would be 4); row 1: the unpenalised argmax
        # is in the history, positive logit (12 / 2 < 8); row 2: every logit negative, the argmax in the history (-10 * 2 = -20)
        "penalty": dict(penalty=2.0, ngram=0, gen=[[A_, B_, A_, C_, 60], [A_, B_, C_, 61, 62], [A_, B_, C_, 61, 62]],
                        plant=[(0, A_, 16.0), (0, FREE, 7.0), (1, B_, 12.0), (1, FREE, 8.0), (2, C_, -10.0)], shift=[0, 0, -20.0],
                        changed=("plain", [1, 2]), picks=("plain", {0: A_, 1: FREE})),
        # n >= g; row 0: one window bans the argmax; row 1: two windows ban two ids; row 2: the window lies in the decoder prompt
        "2-gram": dict(penalty=1.0, ngram=2, gen=[[A_, B_, C_, 61, A_], [A_, B_, A_, C_, A_], [A_, 61, 62, 63, eos + 7]],
                       plant=[(0, B_, 12.0), (0, FREE, 8.0), (1, B_, 12.0), (1, C_, 11.0), (1, FREE, 8.0), (2, 50, 12.0),
                              (2, FREE, 8.0)], shift=[0, 0, 0], changed=("plain", [0, 1, 2]), picks=("plain", {0: FREE, 1: FREE, 2: FREE})),
        # n + 1 < g (n = 9, g = 11): nothing is banned, the history tokens are picked
        "n below g": dict(penalty=1.0, ngram=11, gen=[[A_, B_, C_, A_, B_]] * 3,
                          plant=[(0, C_, 12.0), (1, A_, 12.0), (2, 50, 12.0)], shift=[0, 0, 0], changed=("plain", []),
                          picks=("plain", {0: C_, 1: A_, 2: 50})),
        # both rules, g = 3; row 0: (a, b) was followed by c; row 1: (b, a) never occurred -- c is only penalised (12 / 1.5 = 8 > 7)
        "both": dict(penalty=1.5, ngram=3, gen=[[A_, B_, C_, A_, B_], [A_, B_, C_, B_, A_], [A_, B_, C_, 61, 62]],
                     plant=[(0, C_, 12.0), (0, FREE, 8.0), (1, C_, 12.0), (1, FREE, 7.0), (2, FREE, 9.0)], shift=[0, 0, 0],
                     changed=("plain", [0]), picks=("plain", {0: FREE, 1: C_, 2: FREE})),
        # g = 1 bans every history token, prompt included
        "1-gram": dict(penalty=1.0, ngram=1, gen=[[A_, B_, C_, 61, 62]] * 3,
                       plant=[(0, A_, 12.0), (0, B_, 11.0), (0, FREE, 8.0), (1, 50, 12.0), (1, FREE, 8.0), (2, 700, 12.0)],
                       shift=[0, 0, 0], changed=("plain", [0, 1]), picks=("plain", {0: FREE, 1: FREE, 2: 700})),
        # the first generated position: the history is the decoder prompt
        "first step": dict(penalty=2.0, ngram=1, gen=[[], [], []], plant=[(0, 50, 12.0), (0, FREE, 8.0), (1, FREE, 9.0)],
                           shift=[0, 0, -20.0], changed=("plain", [0]), picks=("plain", {0: FREE, 1: FREE})),
        # timestamp rules; row 0: text + timestamp -- the timestamp may repeat, it is in the history, and its penalty turns the
        # mass rule (10 > 9 = EOS, 10 / 2 < 9); row 1: a closed pair, then text: the penalty moves the best text token; row 2: a
        # finished row
        "timestamp mass": dict(penalty=2.0, ngram=0, gen=[[tb + 5, 41, tb + 20], [tb + 1, tb + 4, 41], [tb + 0, 42, eos]],
                               plant=[(0, tb + 20, 10.0), (0, eos, 9.0), (1, 41, 12.0), (1, FREE, 8.0)], shift=[0, 0, 0],
                               ts_shift=-4.0, done=[0, 0, 1], changed=("timestamps", [0, 1]),
                               picks=("timestamps", {0: eos, 1: FREE, 2: eos})),
        # timestamp rules with an n-gram ban; row 0: text after text, the ban hits the argmax; row 1: a closed pair whose repeat is
        # banned as well as forbidden; row 2: the repeated timestamp is penalised and still the best timestamp
        "timestamp 2-gram": dict(penalty=1.25, ngram=2, gen=[[tb + 2, A_, B_, A_], [tb + 2, A_, tb + 9, tb + 9], [tb + 1, 41, 42, tb + 30]],
                                 plant=[(0, B_, 12.0), (0, FREE, 8.0), (1, A_, 12.0), (1, FREE, 8.0), (2, tb + 30, 10.0),
                                        (2, tb + 40, 7.0), (2, eos, 3.0)], shift=[0, 0, 0], ts_shift=-4.0,
                                 changed=("timestamps", [0]), picks=("timestamps", {0: FREE, 1: A_, 2: tb + 30})),
    }


def _row(V, ld, seed, shift, ts_shift):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(ld, generator=g) * 1.5 + shift
    _, tb = _ids(V)
    x[tb:V] += (torch.rand(1, generator=g).item() - 0.5) * 6.0 if ts_shift is None else ts_shift
    return x


def _inputs(V, ld, case, seeds):
    eos, _ = _ids(V)
    logits = torch.stack([_row(V, ld, seeds[b], case["shift"][b], case.get("ts_shift")) for b in range(B)])
    for b, c, v in case["plant"]:
        logits[b, c] = v
    tokens = torch.zeros(B, LD_TOK, dtype=torch.int64)
    for b in range(B):
        row = [eos + 1, eos + 2, eos + 7, 50] + list(case["gen"][b])
        tokens[b, :len(row)] = torch.tensor(row)
    n = P + len(case["gen"][0])
    done = torch.tensor(case.get("done", [0, 0, 0]), dtype=torch.bool)
    return logits.bfloat16(), tokens, n, done


def _select_kw(V, kw, n):
    eos, _ = _ids(V)
    j = n - P
    return dict(suppress=kw.get("suppress"), begin_suppress=kw.get("begin_suppress"), first=j == 0, no_eos=j < kw.get("min_new", 0),
                ts_begin=kw.get("ts_begin", -1), max_initial=kw.get("max_initial", -1), begin_index=P, eos=kw["eos"], fill=eos)


def _draw(V, ld, case, kw, seed0):
    """inputs whose every decision keeps 1e-3 from a tie / the mass-rule threshold: a row that does not is redrawn"""
    seeds = [seed0 + 1000 * b for b in range(B)]
    for _ in range(20):
        logits, tokens, n, done = _inputs(V, ld, case, seeds)
        skw = _select_kw(V, kw, n)
        want = hr.select_history_ref(logits, V, tokens, n, done=done, repetition_penalty=case["penalty"],
                                     no_repeat_ngram=case["ngram"], **skw)
        close = [b for b in range(B) if want[2][b] < 1e-3 and not bool(done[b])]
        if not close:
            return logits, tokens, n, done, skw, want
        for b in close:
            seeds[b] += 1
    raise AssertionError("rows still within 1e-3 of a tie after 20 redraws")


def _launch(fn, logits, V, tokens, n, done, skw, **opts):
    dl, dt, dd = logits.cuda(), tokens.cuda(), done.cuda()
    cur = torch.full((B, 1), -7, dtype=torch.int64, device="cuda")
    dkw = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in skw.items()}
    fn(dl, V, dt, n, cur, done=dd, **dkw, **opts)
    torch.cuda.synchronize()
    return dt.cpu(), dd.cpu(), cur.cpu()


@pytest.mark.parametrize("V,ld", SHAPES)
def test_kernel_against_the_restatement(ops, V, ld):
    cases = _cases(V)
    for ci, (cname, case) in enumerate(cases.items()):
        for ki, (kname, kw) in enumerate(_configs(V).items()):
            logits, tokens, n, done, skw, (want, want_done, margins) = _draw(V, ld, case, kw, seed0=V + 17 * ci + 5 * ki)
            got_tok, got_done, cur = _launch(ops.greedy_select_history, logits, V, tokens, n, done, skw,
                                             repetition_penalty=case["penalty"], no_repeat_ngram=case["ngram"])
            what = (cname, kname, [f"{m:.3g}" for m in margins])
            assert got_tok[:, n].tolist() == want.tolist(), what
            assert cur[:, 0].tolist() == want.tolist(), what
            assert got_done.tolist() == want_done.tolist(), what
            assert torch.equal(got_tok[:, :n], tokens[:, :n]) and torch.equal(got_tok[:, n + 1:], tokens[:, n + 1:])
            # the case reaches the branch it was written for: the rules change (or keep) the designed rows' tokens
            if kname == case["changed"][0]:
                off, _, _ = hr.select_history_ref(logits, V, tokens, n, done=done, **skw)
                differs = [b for b in range(B) if int(off[b]) != int(want[b])]
                assert set(case["changed"][1]) <= set(differs), (cname, differs)
                for b, t in case["picks"][1].items():
                    assert int(want[b]) == t, (cname, b, int(want[b]), t)


@pytest.mark.parametrize("V,ld", SHAPES)
def test_rules_off_select_what_dw_greedy_select_selects(ops, V, ld):
    for ci, (cname, case) in enumerate(_cases(V).items()):
        for ki, (kname, kw) in enumerate(_configs(V).items()):
            logits, tokens, n, done = _inputs(V, ld, case, [V + 31 * ci + 7 * ki + 1000 * b for b in range(B)])
            skw = _select_kw(V, kw, n)
            a = _launch(ops.greedy_select, logits, V, tokens, n, done, skw)
            b = _launch(ops.greedy_select_history, logits, V, tokens, n, done, skw, repetition_penalty=1.0, no_repeat_ngram=0)
            for x, y in zip(a, b):
                assert torch.equal(x, y), (cname, kname)
    # a forced position copies the prompt token, whatever the options
    tokens = torch.arange(B * LD_TOK, dtype=torch.int64).view(B, LD_TOK).cuda()
    cur = torch.zeros(B, 1, dtype=torch.int64, device="cuda")
    ops.greedy_select_history(None, V, tokens, 2, cur, forced=True, repetition_penalty=1.7, no_repeat_ngram=2)
    assert cur[:, 0].tolist() == tokens[:, 2].tolist()


@pytest.mark.parametrize("name", ["repetition_penalty", "no_repeat_2gram", "no_repeat_1gram", "both", "timestamps_one_window"])
def test_generate_end_to_end_with_graphs_off_and_on(ops, name):
    sc = SC[name]
    model = hr.dropin(ops, sc)
    outs = {}
    for graphs in (False, True):
        outs[graphs] = hr.run(model, sc, device="cuda", use_graphs=graphs)
        assert outs[graphs] == sc["sequences"], f"graphs={graphs}"
        (dec,) = model._decoders.values()
        assert dec.history is not None and dec.use_graphs == graphs
        if graphs:
            assert len(dec.graphs) > 0                    # the token steps really were replayed from HIP graphs
    assert outs[False] == outs[True]
    # a second call replays the captured graphs on a new history
    assert hr.run(model, sc, device="cuda", use_graphs=True) == sc["sequences"]


def test_seek_loop_end_to_end(ops):
    sc = SC["seek_loop"]
    model = hr.dropin(ops, sc)
    assert hr.run(model, sc, device="cuda") == sc["sequences"]
    got = model.generate(hr.inputs_of(sc).cuda(), return_segments=True, **sc["kwargs"])
    assert [[list(s["tokens"]) for s in row] for row in got["segments"]] == [[s["tokens"] for s in row] for row in sc["segments"]]
    assert all(dec.history is not None for dec in model._seek_decoders.values()) and model._seek_decoders
    assert gd.EOS not in [t for row in got["segments"] for s in row for t in s["tokens"]]
