"""TEST INFRASTRUCTURE -- float64 numpy restatement of one beam-search step as the two entries of csrc/beam.hip state it
(`dw_beam_candidates`, `dw_beam_update`; include/dwamd.h), for tests/test_beam_step*.py.  Written from the description of the
reference (`transformers` `_beam_search`, the Whisper logits processors), row by row and utterance by utterance with python loops,
not from the kernels or from decoding.beam_step_torch: the three are compared with each other.
Ties: equal values go to the lower flat index beam * V + token (candidates), to the lower position (the two small merges)."""
import numpy as np

NEG = -1.0e9


def allowed_columns(V, hist, begin_index, *, suppress=None, begin_suppress=None, first=False, no_eos=False, ts_begin=-1,
                    max_initial=-1, eos=0):
    """bool [V]: the columns the rules leave (before the timestamp mass rule).  hist: the row's sequence so far (prompt of
    begin_index tokens included)."""
    ok = np.ones(V, dtype=bool)
    if no_eos:
        ok[eos] = False
    if first and begin_suppress is not None:
        ok &= ~np.asarray(begin_suppress[:V], dtype=bool)
    if suppress is not None:
        ok &= ~np.asarray(suppress[:V], dtype=bool)
    if ts_begin >= 0:
        tb = ts_begin
        ok[tb - 1] = False                                       # <|notimestamps|>
        gen = [int(t) for t in hist[begin_index:]]
        if len(gen) == 0:
            ok[:tb] = False                                      # the first token is a timestamp ...
            if max_initial >= 0:
                ok[tb + max_initial + 1:] = False                # ... at most max_initial steps in
        else:
            last_ts = gen[-1] >= tb
            pen_ts = gen[-2] >= tb if len(gen) >= 2 else True
            if last_ts and pen_ts:
                ok[tb:] = False                                  # a closed pair: text only
            elif last_ts:
                ok[:eos] = False                                 # text + timestamp: a timestamp or EOS
            stamps = [t for t in gen if t >= tb]
            if stamps:
                floor = stamps[-1] if (last_ts and not pen_ts) else stamps[-1] + 1
                ok[tb:floor] = False                             # timestamps never decrease
    return ok


def candidates_ref(logits, tokens, n, run_scores, K, *, begin_index=1, eos=0, ts_begin=-1, **rules):
    """logits [R, V] (any float dtype, taken as float64), tokens int [R, >= n], run_scores [R] -> (val f64 [R, K], tok int [R, K],
    mass_margin f64 [R]: |log-sum-exp of the allowed timestamps - best allowed text| where the mass rule compared, inf elsewhere)."""
    x = np.asarray(logits, dtype=np.float64)
    R, V = x.shape
    val = np.full((R, K), -np.inf)
    tok = np.full((R, K), eos, dtype=np.int64)
    margin = np.full(R, np.inf)
    for r in range(R):
        m = x[r].max()
        lse = m + np.log(np.exp(x[r] - m).sum())
        ok = allowed_columns(V, np.asarray(tokens[r][:n]), begin_index, eos=eos, ts_begin=ts_begin, **rules)
        if ts_begin >= 0 and ok[ts_begin:].any():
            ts = x[r, ts_begin:][ok[ts_begin:]]
            ts_lse = ts.max() + np.log(np.exp(ts - ts.max()).sum())
            text = x[r, :ts_begin][ok[:ts_begin]]
            text_max = text.max() if text.size else -np.inf
            margin[r] = abs(ts_lse - text_max)
            if ts_lse > text_max:
                ok[:ts_begin] = False
        cols = np.nonzero(ok)[0]
        v = x[r, cols] - lse + float(run_scores[r])
        order = np.lexsort((cols, -v))[:K]
        val[r, :len(order)] = v[order]
        tok[r, :len(order)] = cols[order]
    return val, tok, margin


def update_ref(st, cand_val, cand_tok, *, k, V, cur, P, max_length, eos, early_stopping, length_penalty):
    """st: dict(running, sequences int [B, k, L]; run_scores, beam_scores f64 [B, k]; finished bool [B, k]; lengths int [B, k];
    unsat bool [B]) -> (new state, src_rows int [B * k], next_tok int [B * k], stop bool).  cand_*: [B * k, K]."""
    B = st["running"].shape[0]
    K = 2 * k
    new = {name: np.array(v, copy=True) for name, v in st.items()}
    new["run_scores"] = new["run_scores"].astype(np.float64)
    new["beam_scores"] = new["beam_scores"].astype(np.float64)
    src_rows = np.zeros(B * k, dtype=np.int64)
    next_tok = np.zeros(B * k, dtype=np.int64)
    fin_div = float((cur + 1 - P) ** length_penalty)
    hyp_len = (max_length - P) if (early_stopping == "never" and length_penalty > 0.0) else (cur + 1 - P)
    hyp_div = float(hyp_len ** length_penalty)
    all_hits = True
    for u in range(B):
        cv = np.asarray(cand_val[u * k:(u + 1) * k], dtype=np.float64).reshape(-1)
        ct = np.asarray(cand_tok[u * k:(u + 1) * k], dtype=np.int64).reshape(-1)
        flat = np.repeat(np.arange(k), K) * V + ct
        order = np.lexsort((np.arange(k * K), flat, -cv))[:K]
        top_lp, src_beam, tok = cv[order], flat[order] // V, flat[order] % V
        hits = (tok == eos) | (cur + 1 >= max_length)
        all_hits &= bool(hits.all())
        open_lp = np.where(hits, top_lp + NEG, top_lp)
        nxt = np.lexsort((np.arange(K), -open_lp))[:k]
        for r, j in enumerate(nxt):
            row = np.array(st["running"][u, src_beam[j]], copy=True)
            row[cur] = tok[j]
            new["running"][u, r] = row
            new["run_scores"][u, r] = open_lp[j]
            src_rows[u * k + r] = u * k + src_beam[j]
            next_tok[u * k + r] = tok[j]
        just = hits & (np.arange(K) < k)
        fin_lp = top_lp / fin_div
        if st["finished"][u].all() and early_stopping is True:
            fin_lp = fin_lp + NEG
        if not st["unsat"][u]:
            fin_lp = fin_lp + NEG
        fin_lp = np.where(just, fin_lp, fin_lp + NEG)
        m_sc = np.concatenate([np.asarray(st["beam_scores"][u], dtype=np.float64), fin_lp])
        best = np.lexsort((np.arange(k + K), -m_sc))[:k]
        for r, j in enumerate(best):
            if j < k:
                new["sequences"][u, r] = st["sequences"][u, j]
                new["finished"][u, r] = st["finished"][u, j]
                new["lengths"][u, r] = st["lengths"][u, j]
            else:
                row = np.array(st["running"][u, src_beam[j - k]], copy=True)
                row[cur] = tok[j - k]
                new["sequences"][u, r] = row
                new["finished"][u, r] = just[j - k]
                new["lengths"][u, r] = cur + 1 - P
            new["beam_scores"][u, r] = m_sc[j]
        best_running = new["run_scores"][u, 0] / hyp_div
        worst = np.where(new["finished"][u], new["beam_scores"][u].min(), NEG)
        new["unsat"][u] = bool(st["unsat"][u]) and bool((best_running > worst).any())
    go_on = bool(new["unsat"].any()) and not (bool(new["finished"].all()) and early_stopping is True) and not all_hits
    return new, src_rows, next_tok, not go_on


def step_ref(st, logits, *, k, V, cur, P, max_length, eos, early_stopping=False, length_penalty=1.0, min_new_tokens=0,
             suppress=None, begin_suppress=None, ts_begin=-1, max_initial=-1, begin_index=None):
    """candidates + update.  -> (new state, src_rows, next_tok, stop, (cand_val, cand_tok, mass_margin))."""
    B = st["running"].shape[0]
    tokens = np.asarray(st["running"]).reshape(B * k, -1)
    cand = candidates_ref(logits, tokens, cur, np.asarray(st["run_scores"], dtype=np.float64).reshape(-1), 2 * k,
                          begin_index=P if begin_index is None else begin_index, eos=eos, ts_begin=ts_begin, suppress=suppress,
                          begin_suppress=begin_suppress, first=(cur == P), no_eos=(cur - P) < min_new_tokens,
                          max_initial=max_initial)
    new, src_rows, next_tok, stop = update_ref(st, cand[0], cand[1], k=k, V=V, cur=cur, P=P, max_length=max_length, eos=eos,
                                               early_stopping=early_stopping, length_penalty=length_penalty)
    return new, src_rows, next_tok, stop, cand
