"""TEST INFRASTRUCTURE -- one round of speculative (assisted) greedy decoding restated in numpy float64, from the reference's
documentation of its logits processors and of `_assisted_decoding` (third-party `transformers`), independent of
decoding.assist_pick_torch / assist_accept_torch and of csrc/assist.hip: the token the rules pick at k + 1 consecutive positions
of every row, then the accept step (agreeing prefix, minimum over the rows, EOS / pad bookkeeping)."""
import numpy as np

NEG = -np.inf


def _lse(x):
    m = np.max(x) if x.size else NEG
    if not np.isfinite(m):
        return NEG
    return m + np.log(np.sum(np.exp(x - m)))


def processed_row(logit, hist, P0, eos=None, min_new=0, suppress=(), begin_suppress=(), ts=None):
    """The processed scores f64 [V] of the position len(hist) of one row (hist: the whole sequence so far, prompt of P0 tokens
    included) and the margin |logsumexp(timestamps) - max(text)| of the mass rule (inf where it is not evaluated).
    ts: dict(no_timestamps_token_id, max_initial_timestamp_index) or None."""
    sc = np.array(logit, dtype=np.float64)
    n_gen = len(hist) - P0
    if eos is not None and n_gen < min_new:
        sc[eos] = NEG
    if n_gen == 0:
        sc[list(begin_suppress)] = NEG
    sc[list(suppress)] = NEG
    margin = np.inf
    if ts is not None:
        tb = ts["no_timestamps_token_id"] + 1
        sc[tb - 1] = NEG
        seq = [int(t) for t in hist[P0:]]
        if n_gen >= 1:
            last_ts = seq[-1] >= tb
            pen_ts = seq[-2] >= tb if n_gen >= 2 else True
            if last_ts and pen_ts:
                sc[tb:] = NEG                                        # a closed pair: text only
            elif last_ts:
                sc[:eos] = NEG                                       # text + timestamp: a timestamp or EOS
            stamps = [t for t in seq if t >= tb]
            if stamps:
                lo = stamps[-1] if (last_ts and not pen_ts) else stamps[-1] + 1
                sc[tb:lo] = NEG                                      # timestamps never decrease
        else:
            sc[:tb] = NEG                                            # the first token is a timestamp
            mi = ts.get("max_initial_timestamp_index")
            if mi is not None:
                sc[tb + mi + 1:] = NEG
        lse_all = _lse(sc)
        ts_lp, text_max = _lse(sc[tb:]) - lse_all, np.max(sc[:tb]) - lse_all
        if np.isfinite(ts_lp) or np.isfinite(text_max):
            margin = abs(ts_lp - text_max) if (np.isfinite(ts_lp) and np.isfinite(text_max)) else np.inf
        if ts_lp > text_max:
            sc[:tb] = NEG
    return sc, margin


def pick_ref(logits, tokens, L, P0, eos=None, min_new=0, suppress=(), begin_suppress=(), ts=None):
    """logits f64 [B, n, V]: row (b, j) predicts tokens[b, L + j] from tokens[b, :L + j] -> (own int64 [B, n], smallest mass-rule
    margin met).  Among equal scores the lower column (np.argmax)."""
    B, n, _ = logits.shape
    own = np.zeros((B, n), dtype=np.int64)
    worst = np.inf
    for b in range(B):
        for j in range(n):
            sc, m = processed_row(logits[b, j], tokens[b, :L + j], P0, eos, min_new, suppress, begin_suppress, ts)
            own[b, j] = int(np.argmax(sc))
            worst = min(worst, m)
    return own, worst


def accept_ref(own, tokens, L, k, done, eos=None, fill=None):
    """-> (tokens, done, n_ok, all_done) after the round: own int64 [B, k + 1], the k drafts at tokens[:, L:L + k]."""
    tokens, done = tokens.copy(), done.copy()
    B = own.shape[0]
    n_ok = k
    for b in range(B):
        m = 0
        if eos is not None and done[b]:
            m = k
        else:
            while m < k and own[b, m] == tokens[b, L + m]:
                m += 1
        n_ok = min(n_ok, m)
    for b in range(B):
        for j in range(n_ok + 1):
            c = own[b, j]
            if eos is not None:
                if done[b]:
                    c = fill
                if c == eos:
                    done[b] = True
            tokens[b, L + j] = c
    return tokens, done, n_ok, bool(eos is not None and done.all())
