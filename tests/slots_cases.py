"""TEST INFRASTRUCTURE -- inputs and the numpy restatement of the slot step of continuous batching (tests/test_slots*.py).

`slot_step_ref` is written from the rule as include/dwamd.h states it for `dw_slot_step`, independent of decoding.slot_step_torch
and of csrc/slots.hip; the scores are judged by the float64 statement of the logits rules in tests/assist_restatement.py
(`processed_row`), imported, not copied.

`make_launch` puts one planted single-row case of tests/assist_cases.py per slot side by side -- each slot with its own prompt
length, history length and state -- so that one launch meets: a slot inside its prompt, slots at the first generated position,
every timestamp state of `assist_cases.scenarios`, min_new_tokens crossing in one slot only, a slot emitting EOS, one reaching its
budget, one already done.  The planted columns decide every token at least 0.25 above the next (assist_cases)."""
import numpy as np

from tests import assist_cases as ac
from tests.assist_restatement import processed_row

MIN_NEW = 3
MAX_LEN = 16


def slot_step_ref(logits, tokens, length, plen, budget, done, eos, min_new=0, suppress=(), begin_suppress=(), ts=None):
    """-> (tokens, length, done, row_t, cur, smallest mass-rule margin) after one slot step.  logits f64 [S, V]."""
    tokens, length, done = tokens.copy(), np.array(length, dtype=np.int64), np.array(done, dtype=bool)
    S = tokens.shape[0]
    row_t, cur = np.zeros(S, dtype=np.int64), np.zeros(S, dtype=np.int64)
    worst = np.inf
    for b in range(S):
        n, P = int(length[b]), int(plen[b])
        if done[b]:
            row_t[b], cur[b] = 0, tokens[b, 0]             # parked at position 0, the row left alone
            continue
        generated = n >= P
        if generated:
            sc, m = processed_row(logits[b], tokens[b, :n], P, eos, min_new, suppress, begin_suppress, ts)
            nxt = int(np.argmax(sc))
            second = np.partition(sc, -2)[-2]
            assert sc[nxt] - second >= 0.25, (b, sc[nxt], second)           # decided before any implementation runs
            worst = min(worst, m)
        else:
            nxt = int(tokens[b, n])                        # teacher forcing
        tokens[b, n] = nxt
        length[b] = n + 1
        if generated and (nxt == eos or n + 1 >= budget[b]):
            done[b] = True
            row_t[b], cur[b] = 0, tokens[b, 0]
        else:
            row_t[b], cur[b] = n, nxt
    return tokens, length, done, row_t, cur, worst


def _slots(ts):
    """(name, scenario of assist_cases, overrides, n_hist, P0, state) per slot; prompt lengths differ between slots."""
    text = "all_accepted"
    eos_first = dict(prefer=["eos"])
    out = [("prompt", text, {}, 0, 5, "prompt"),
           ("eos", text, eos_first, 5, 3, "gen"),                       # n - plen >= MIN_NEW: EOS is taken, the slot ends
           ("min_new", text, eos_first, MIN_NEW - 1, 4, "gen"),         # the same planted row one token short of MIN_NEW: EOS excluded
           ("budget", text, {}, 4, 2, "budget"),
           ("done", text, {}, 4, 3, "done"),
           ("suppress", "suppress", {}, 6, 1, "gen")]
    if ts:
        out += [("ts_first", "ts_first", {}, 0, 4, "gen"), ("ts_text_ts", "ts_text_ts", {}, 5, 3, "gen"),
                ("ts_pair", "ts_pair", {}, 6, 2, "gen"), ("ts_open", "ts_open", {}, 4, 5, "gen"),
                ("ts_mass_taken", "ts_mass_taken", {}, 5, 3, "gen"), ("ts_mass_not_taken", "ts_mass_not_taken", {}, 4, 4, "gen")]
    else:
        out += [("first", text, dict(first=True), 0, 4, "gen"), ("first_long_prompt", text, dict(first=True), 0, 6, "gen")]
    return out


def make_launch(V, ts, seed=0):
    """-> dict(names, logits f64 [S, V] of bf16-exact values, tokens int64 [S, MAX_LEN], length, plen, budget, done, eos, min_new,
    suppress, begin_suppress (ids), ts (rules dict or None), want = slot_step_ref's output)."""
    specs = _slots(ts)
    S = len(specs)
    logits = np.zeros((S, V))
    tokens = np.full((S, MAX_LEN), 7, dtype=np.int64)                   # 7: a sentinel text id behind the row
    length, plen, budget, done = (np.zeros(S, dtype=np.int64) for _ in range(4))
    suppress, rules, eos = set(), None, None
    for b, (name, scen, over, n_hist, P0, state) in enumerate(specs):
        sc = dict(ac.scenarios(1, 0)[scen], **over)
        if ts and not sc["ts"]:
            sc = dict(sc, ts=True, kind="open" if n_hist else "text")    # the rules are on for the whole launch
        for attempt in range(40):                                        # first seed whose mass-rule margins are clear
            try:
                c = ac.make_case(seed + 1000 * attempt + 31 * b + V, V, 1, 0, sc, n_hist=max(n_hist, 1), P0=P0, pad_behind=0)
                break
            except AssertionError:
                continue
        else:
            raise AssertionError(f"no clear-margin case for slot {name}")
        L = P0 if (sc["first"] or n_hist == 0) else c["L"]
        tokens[b, :L] = c["tokens"][0, :L]
        logits[b] = c["logits"][0, 0]
        length[b], plen[b], budget[b] = L, P0, P0 + 9
        suppress |= set(c["suppress"])
        eos, rules = c["eos"], (c["ts"] if ts else None)
        if state == "prompt":
            length[b] = 2                                                # position 2 of a prompt of five
        elif state == "budget":
            budget[b] = L + 1
        elif state == "done":
            done[b] = 1
    if rules is not None:
        rules = dict(no_timestamps_token_id=rules["no_timestamps_token_id"], max_initial_timestamp_index=rules["max_initial_timestamp_index"])
    # the best column of the first-position slot of the launch without timestamp rules is begin-suppressed: it counts there only
    begin_suppress = []
    if not ts:
        b = [s[0] for s in specs].index("first")
        begin_suppress = [int(np.argmax(processed_row(logits[b], tokens[b, :length[b]], plen[b], eos, MIN_NEW, sorted(suppress))[0]))]
    kw = dict(eos=eos, min_new=MIN_NEW, suppress=sorted(suppress), begin_suppress=begin_suppress, ts=rules)
    want = slot_step_ref(logits, tokens, length, plen, budget, done.astype(bool), **kw)
    assert want[5] > 0.25, want[5]
    return dict(names=[s[0] for s in specs], logits=logits, tokens=tokens, length=length, plen=plen, budget=budget,
                done=done.astype(bool), want=want, **kw)


def check_launch(c, tokens, length, done, row_t, cur):
    """The state after the step under test (arrays / lists) against the restatement; every integer is exact.  Also what the cases
    were planted for."""
    w_tok, w_len, w_done, w_rt, w_cur, _ = c["want"]
    assert np.asarray(tokens).tolist() == w_tok.tolist()
    assert list(length) == w_len.tolist() and [bool(x) for x in done] == w_done.tolist()
    assert list(row_t) == w_rt.tolist() and [int(x) for x in np.asarray(cur).reshape(-1)] == w_cur.tolist()
    at = {n: i for i, n in enumerate(c["names"])}
    eos = c["eos"]
    b = at["prompt"]
    assert w_tok[b, 2] == c["tokens"][b, 2] and w_len[b] == 3 and not w_done[b] and w_rt[b] == 2
    b = at["eos"]
    assert w_tok[b, c["length"][b]] == eos and w_done[b] and w_rt[b] == 0 and w_cur[b] == c["tokens"][b, 0]
    b = at["min_new"]
    assert w_tok[b, c["length"][b]] != eos and not w_done[b]
    b = at["budget"]
    assert w_done[b] and w_len[b] == c["budget"][b] and w_tok[b, c["length"][b]] != eos
    b = at["done"]
    assert w_tok[b].tolist() == c["tokens"][b].tolist() and w_len[b] == c["length"][b] and w_rt[b] == 0
    assert len(set(c["plen"].tolist())) >= 4
    if c["ts"] is not None:
        tb = c["ts"]["no_timestamps_token_id"] + 1
        new = {n: int(w_tok[i, c["length"][i]]) for n, i in at.items()}
        assert new["ts_first"] in (tb, tb + 1) and new["ts_pair"] < tb and new["ts_text_ts"] >= eos
        assert new["ts_mass_taken"] >= tb and new["ts_mass_not_taken"] < tb
    else:
        assert int(w_tok[at["first"], c["length"][at["first"]]]) != c["begin_suppress"][0]
