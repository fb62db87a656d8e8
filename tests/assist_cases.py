"""TEST INFRASTRUCTURE -- planted rounds of speculative decoding for tests/test_assist*.py.

Every logits row is bf16 noise in [-4, 4] plus NPL planted columns (values exact in bf16) drawn from the regions text / EOS /
timestamps: the first, in the region the scenario prefers at that position, at 16; the other text / EOS columns at 12 + 0.25 r, the
other timestamps at 8 + 0.25 r (r < NPL, each r once).  Whichever planted column the rules leave is the row's token, at least 0.25
above the next and 4 above the noise, and the mass rule is never near its threshold (timestamps without the 16 sum to below 10.5,
under every planted text column; a timestamp at 16 is above them all), so the integers are decided before any implementation runs.
At a first position with max_initial = 1 the two allowed timestamps are planted at 9 and 9.5.  The mass rule is planted on its own (`mass`): taken -- best text 10, timestamps 9.75, 9.5, 9.25, 9 (logsumexp 10.8); not
taken -- best text 16 against timestamp noise (logsumexp < 4 + ln 1501 = 11.4).  The drafts are derived position by position from
tests/assist_restatement.py: row b agrees with the target up to `reject[b]` and holds another text token from there on."""
import numpy as np

from tests.assist_restatement import pick_ref
from tests.beam_cases import bf16_round, history, layout

NPL = 6


def scenarios(B, k):
    """name -> dict(reject=[per row], done=[per row], prefer=[per position], kind=, ts=, first=, min_new_in=, suppress_top=, mass=)"""
    mid = k // 2
    differ = [k, min(1, k), min(3, k)][:B]
    base = dict(reject=[k] * B, done=[False] * B, prefer=["text"] * (k + 1), kind="text", ts=False, first=False, min_new_in=None,
                suppress_top=False, mass=None)
    out = {
        "all_accepted": {},
        "reject_first": dict(reject=[0] * B),
        "reject_middle": dict(reject=[mid] * B),
        "rows_differ": dict(reject=differ),
        "done_row": dict(done=[i == B - 1 for i in range(B)], reject=[k] * (B - 1) + [0]),
        "eos_accepted": dict(prefer=["text", "eos", "text", "text", "text", "text"][:k + 1]),
        "min_new_inside": dict(prefer=["eos"] * (k + 1), min_new_in=min(2, k)),
        "suppress": dict(suppress_top=True),
        "ts_first": dict(ts=True, first=True, prefer=["ts", "text", "text", "ts", "ts", "text"][:k + 1]),
        "ts_text_ts": dict(ts=True, kind="text_ts", prefer=["text", "ts", "text", "text", "ts", "ts"][:k + 1]),
        "ts_pair": dict(ts=True, kind="pair", prefer=["ts", "text", "ts", "ts", "ts", "text"][:k + 1]),
        "ts_open": dict(ts=True, kind="open", prefer=["ts", "ts", "text", "ts", "eos", "text"][:k + 1], reject=differ),
        "ts_mass_taken": dict(ts=True, kind="open", mass="taken"),
        "ts_mass_not_taken": dict(ts=True, kind="open", mass="not_taken"),
    }
    return {n: {**base, **v} for n, v in out.items()}


def make_case(seed, V, B, k, sc, n_hist=5, P0=3, pad_behind=2):
    """-> dict(logits f64 [B, k + 1, V] of bf16-exact values, tokens int64 [B, L + k + 1 + pad_behind] -- prompt, history, the k
    drafts, then a sentinel --, L, P0, done, eos, fill, min_new, suppress (ids), ts (rules dict or None), own (expected))."""
    rng = np.random.default_rng(seed)
    lay = layout(V)
    tb, eos, nots = lay["tb"], lay["eos"], lay["nots"]
    L = P0 if sc["first"] else P0 + n_hist
    n = k + 1
    tok_ld = L + n + pad_behind
    tokens = np.full((B, tok_ld), 7, dtype=np.int64)          # 7: a sentinel text id behind the round
    tokens[:, :P0] = rng.integers(eos + 1, nots, size=(B, P0)) if nots > eos + 1 else eos
    for b in range(B):
        if L > P0:
            tokens[b, P0:L] = history(sc["kind"] if sc["ts"] else "text", lay, rng, L - P0)
    ts = dict(begin_index=P0, no_timestamps_token_id=nots, max_initial_timestamp_index=1) if sc["ts"] else None
    x = bf16_round(np.clip(rng.normal(0.0, 1.0, size=(B, n, V)), -4.0, 4.0))
    suppress = []
    regions = {"text": (8, eos), "eos": (eos, eos + 1), "ts": (tb, V)}
    for b in range(B):
        for j in range(n):
            if sc["mass"] is not None:
                t = int(rng.integers(8, eos))
                if sc["mass"] == "taken":
                    x[b, j, t] = 10.0
                    cols = tb + 20 + rng.choice(V - tb - 20, size=4, replace=False)
                    x[b, j, cols] = [9.75, 9.5, 9.25, 9.0]
                else:
                    x[b, j, t] = 16.0
                continue
            order = [sc["prefer"][j]] + [("text", "ts", "eos", "text", "ts")[(i + j) % 5] for i in range(NPL - 1)]
            used = set()
            for r, reg in enumerate(order):
                lo, hi = regions[reg]
                if reg == "ts":                                # spread over early and late timestamps
                    lo, hi = (tb, tb + 12) if r % 2 else (tb + 12, V)
                c = int(rng.integers(lo, hi))
                if c in used or c == nots:
                    continue
                used.add(c)
                # the preferred column far above the rest; the other text columns above every timestamp's mass
                x[b, j, c] = 16.0 if r == 0 else (8.0 if reg == "ts" else 12.0) + 0.25 * (NPL - 1 - r)
                if r == 0 and sc["suppress_top"]:
                    suppress.append(c)
            if sc["first"] and j == 0:                         # only tb and tb + 1 are allowed there (max_initial = 1)
                x[b, j, tb], x[b, j, tb + 1] = 9.0, 9.5
    min_new = 0 if sc["min_new_in"] is None else (L - P0) + sc["min_new_in"]
    done = np.array(sc["done"], dtype=bool)
    fill = eos + 1 if nots > eos + 1 else eos                  # a pad id that is not EOS where the layout has room
    # drafts, position by position: the history of position j holds the drafts before it
    kw = dict(eos=eos, min_new=min_new, suppress=sorted(set(suppress)), ts=ts)
    margin = np.inf
    for j in range(k):
        own_j, m = pick_ref(x[:, j:j + 1], tokens, L + j, P0, **kw)
        margin = min(margin, m)
        for b in range(B):
            other = 9 if own_j[b, 0] != 9 else 10
            tokens[b, L + j] = own_j[b, 0] if j < sc["reject"][b] else other
    own, m = pick_ref(x, tokens, L, P0, **kw)
    margin = min(margin, m)
    assert margin > 0.25, margin                               # the mass rule is never near its threshold
    return dict(logits=x, tokens=tokens, L=L, P0=P0, k=k, done=done, eos=eos, fill=fill, min_new=min_new,
                suppress=sorted(set(suppress)), ts=ts, own=own, lay=lay)
