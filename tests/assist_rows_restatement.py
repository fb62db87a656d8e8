"""TEST INFRASTRUCTURE -- one round of speculative decoding with PER-ROW acceptance restated in numpy: every row stands at its own
length, agrees with the target on its own draft prefix and ends at its own EOS.  The scores are judged by the float64 statement of
the logits rules in tests/assist_restatement.py (`processed_row`), imported, not copied; the bookkeeping below is written from the
rule as include/dwamd.h states it for `dw_assist_accept_rows`, independent of decoding.assist_accept_rows_torch and of
csrc/assist.hip."""
import numpy as np

from tests.assist_restatement import processed_row


def pick_rows_ref(logits, tokens, lens, j0, P0, eos=None, min_new=0, suppress=(), begin_suppress=(), ts=None):
    """logits f64 [B, n, V]: row (b, j) predicts tokens[b, lens[b] + j0 + j] from tokens[b, :lens[b] + j0 + j] -> (own int64 [B, n],
    smallest mass-rule margin met).  A position behind the buffer is not judged: 0.  Among equal scores the lower column."""
    B, n, _ = logits.shape
    own = np.zeros((B, n), dtype=np.int64)
    worst = np.inf
    for b in range(B):
        for j in range(n):
            at = int(lens[b]) + j0 + j
            if at >= tokens.shape[1]:
                continue
            sc, m = processed_row(logits[b, j], tokens[b, :at], P0, eos, min_new, suppress, begin_suppress, ts)
            own[b, j] = int(np.argmax(sc))
            worst = min(worst, m)
    return own, worst


def accept_rows_ref(own, tokens, lens, k, total, done, eos=None, fill=0):
    """-> (tokens, lens, done, pos_target, pos_assistant, result) after the round.  own int64 [B, k + 1]; row b's k drafts stand at
    tokens[b, lens[b]:lens[b] + k]; result = [drafts accepted, drafts offered, every row done, largest live length]."""
    tokens, lens, done = tokens.copy(), np.array(lens, dtype=np.int64), np.array(done, dtype=bool)
    B = own.shape[0]
    pos_t, pos_a = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
    accepted = offered = 0
    for b in range(B):
        start = int(lens[b])
        last = min(start + k, total - 1)                    # where this round's drafts (or the target's token) can have reached
        if not done[b] and start < total:
            drafts = tokens[b, start:last].tolist()         # the kb = last - start drafts offered to this row
            offered += len(drafts)
            agree = 0
            for d, o in zip(drafts, own[b]):
                if d != o:
                    break
                agree += 1
            new = own[b, :agree + 1].tolist()               # the agreeing drafts and the target's own next token
            if eos is not None and eos in new:
                new = new[:new.index(eos) + 1]              # the row ends behind its EOS
                done[b] = True
            accepted += min(len(new), agree)
            tokens[b, start:start + len(new)] = new
            lens[b] = start + len(new)
            if lens[b] >= total:
                done[b] = True
        elif start >= total:
            done[b] = True
        if done[b]:
            tokens[b, lens[b]:last + 1] = fill              # the drafts behind the row's end
        else:
            pos_t[b], pos_a[b] = lens[b] - 1, lens[b] - 2
    live = [int(lens[b]) for b in range(B) if not done[b]]
    return tokens, lens, done, pos_t, pos_a, [accepted, offered, int(not live), max(live, default=0)]
