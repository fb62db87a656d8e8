"""TEST INFRASTRUCTURE -- beam-search states and logits for tests/test_beam_step*.py: random small states for the CPU comparison
of decoding.beam_step_torch with tests/beam_restatement.py, and planted-logit states for the kernels of csrc/beam.hip.

Planted logits: every row is bf16 noise in [-4, 4] plus 3K planted columns at 8 + 0.25 k j (j < 3K; exact in bf16), and the
running score of beam b is chosen so that `run_score - lse` is -(largest planted value) - 4 + 0.25 b: all k * 3K accumulated scores
of an utterance are negative and at least 0.25 apart (up to the fp32 rounding of the running score), so no selection depends on a
tie or on rounding.  At a first step the running scores stay [0, -1e9, ...]: only beam 0 counts there."""
import numpy as np

NEG = -1.0e9


def layout(V):
    """Token ids of a Whisper-like vocabulary of V columns: text [0, eos), eos, a few specials, <|notimestamps|>, timestamps."""
    n_ts = 1501 if V > 40000 else (200 if V > 500 else max(4, V // 4))
    tb = V - n_ts
    return dict(tb=tb, nots=tb - 1, eos=tb - (8 if V > 500 else 2))


def history(kind, lay, rng, n_gen):
    """n_gen generated tokens that put the timestamp rules into state `kind`."""
    tb, eos = lay["tb"], lay["eos"]
    text = lambda: int(rng.integers(0, eos))
    if kind == "text":                                   # no timestamp in the history (rules off, or before any timestamp)
        return [text() for _ in range(n_gen)]
    if kind == "open":                                   # <ts> text ... text: text or a later timestamp may follow
        return [tb + 3] + [text() for _ in range(n_gen - 1)]
    if kind == "text_ts":                                # ... text <ts>: a timestamp (not smaller) or EOS
        return [tb + 2] + [text() for _ in range(n_gen - 2)] + [tb + 7]
    if kind == "pair":                                   # ... <ts> <ts>: text only
        return [tb + 2] + [text() for _ in range(n_gen - 3)] + [tb + 7, tb + 7]
    raise ValueError(kind)


def make_state(rng, B, k, L, P, cur, lay, kind="text", n_finished=0, first=False, fill=None):
    """A consistent search state at position cur (numpy; the dict of beam_restatement.update_ref)."""
    fill = lay["eos"] if fill is None else fill
    running = np.full((B, k, L), fill, dtype=np.int64)
    sequences = np.full((B, k, L), fill, dtype=np.int64)
    prompt = rng.integers(lay["eos"] + 1, lay["nots"], size=(B, P)) if lay["nots"] > lay["eos"] + 1 else np.full((B, P), lay["eos"])
    running[:, :, :P] = prompt[:, None, :]
    sequences[:, :, :P] = prompt[:, None, :]
    for u in range(B):
        for b in range(k):
            running[u, b, P:cur] = history(kind, lay, rng, cur - P) if cur > P else []
    run_scores = -np.sort(rng.uniform(0.05, 1.0, size=(B, k)), axis=1)
    if first:
        run_scores[:] = NEG
        run_scores[:, 0] = 0.0
    beam_scores = np.full((B, k), NEG)
    finished = np.zeros((B, k), dtype=bool)
    lengths = np.zeros((B, k), dtype=np.int64)
    for u in range(B):
        nf = min(n_finished, k)
        beam_scores[u, :nf] = -np.sort(rng.uniform(0.3, 2.0, size=nf))
        finished[u, :nf] = True
        for b in range(nf):
            n = int(rng.integers(1, max(2, cur - P + 1)))
            lengths[u, b] = n
            sequences[u, b, P:P + n - 1] = rng.integers(0, lay["eos"], size=n - 1)
            sequences[u, b, P + n - 1] = lay["eos"]
    return dict(running=running, sequences=sequences, run_scores=run_scores.astype(np.float32).astype(np.float64),
                beam_scores=beam_scores.astype(np.float32).astype(np.float64), finished=finished, lengths=lengths,
                unsat=np.ones(B, dtype=bool))


def bf16_round(x):
    import torch
    return torch.from_numpy(np.asarray(x, dtype=np.float32)).to(torch.bfloat16).to(torch.float64).numpy()


def planted_logits(rng, st, k, V, lay, regions, top_cols=None, keep_run=False):
    """-> (logits f64 [R, V] of bf16-exact values, run_scores f64 [B, k] of fp32-exact values).  regions: list of (lo, hi) id ranges
    the 3K planted columns of each row are drawn from, in turn; top_cols: {(row or None) -> {rank j: column}} pins the column that
    holds the planted value of rank j (0 = the row's largest)."""
    B = st["running"].shape[0]
    K = 2 * k
    R = B * k
    x = bf16_round(np.clip(rng.normal(0.0, 1.0, size=(R, V)), -4.0, 4.0))
    n_pl = 3 * K
    vals = 8.0 + 0.25 * k * np.arange(n_pl)[::-1]       # rank 0 first
    assert np.array_equal(vals, bf16_round(vals))
    run = np.array(st["run_scores"], copy=True).reshape(-1)
    for r in range(R):
        pinned = dict((top_cols or {}).get(None, {}))
        pinned.update((top_cols or {}).get(r, {}))
        cols, used = [None] * n_pl, set(pinned.values())
        for j, c in pinned.items():
            cols[j] = c
        for j in range(n_pl):
            if cols[j] is None:
                lo, hi = regions[j % len(regions)]
                while True:
                    c = int(rng.integers(lo, hi))
                    if c not in used:
                        break
                used.add(c)
                cols[j] = c
        x[r, cols] = vals
        if not keep_run:
            m = x[r].max()
            lse = m + np.log(np.exp(x[r] - m).sum())
            run[r] = np.float64(np.float32(lse - vals[0] - 4.0 + 0.25 * (r % k)))
    return x, run.reshape(B, k)


def step_margin(decoding, st, logits, cur, cfg):
    """The smallest non-zero gap among the top 2k + 1 accumulated scores per utterance that `decoding.beam_step_torch` is about to
    select from (its masks restated on a copy; nothing of `st` changes).  Pairs inside the -1e9 sentinels do not count, and equal
    scores do not either: both paths decide them by the tie rule (bf16 logits give one beam's columns equal scores all the time)."""
    import torch
    B, nb = st["run_scores"].shape
    sc = torch.log_softmax(logits.float(), -1)
    if cur - cfg["P"] < cfg["min_new_tokens"]:
        sc[:, cfg["eos"]] = float("-inf")
    if cur == cfg["P"] and cfg["bsup"] is not None:
        sc = sc.masked_fill(cfg["bsup"][None, :], float("-inf"))
    if cfg["sup"] is not None:
        sc = sc.masked_fill(cfg["sup"][None, :], float("-inf"))
    tr = cfg["timestamp_rules"]
    if tr is not None:
        flat = st["running"][:, :, :cur].reshape(B * nb, cur)
        sc = decoding.apply_timestamp_rules(sc, flat, cur, tr["begin_index"], tr["no_timestamps_token_id"], cfg["eos"],
                                            tr.get("max_initial_timestamp_index"))
    acc = (sc.view(B, nb, -1) + st["run_scores"][:, :, None]).reshape(B, -1)
    top = torch.topk(acc, 2 * nb + 1)[0]
    gap = (top[:, :-1] - top[:, 1:])[top[:, :-1] > -1.0e8]
    gap = gap[torch.isfinite(gap) & (gap > 0)]
    return float(gap.min()) if gap.numel() else float("inf")
