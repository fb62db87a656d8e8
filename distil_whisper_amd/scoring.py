"""Per-step scores of finished sequences: host side of `generate(output_scores=True / output_logits=True,
return_dict_in_generate=True)` and of `compute_transition_scores`.

The reference (`GenerationMixin._sample`, TF:generation/utils.py; `TF:` = the pinned transformers 5.15.0) keeps, for every decoding
step, the logits after the logits processors (`scores`) and before them (`logits`), one [batch, vocab] fp32 tensor per step;
`compute_transition_scores` gathers the chosen tokens' entries, and the long-form code averages them
(`_retrieve_avg_logprobs`, TF:models/whisper/generation_whisper.py:1958-1975).
Here the graph-captured token step is left alone: one teacher-forced decoder pass over the finished sequences (engine.decode --
the same function of the same token prefix) gives the logits of every step at once, and one kernel (csrc/score.hip) applies the
processors to all (step, row) pairs and also returns each chosen token's score and log-probability.

A SECOND pass: the token step multiplies one row per sequence (GEMV kernels), this pass a block of rows (GEMM kernels); their fp32
sums run in different orders and round differently in bf16.  The values agree to bf16 precision, but on a near tie
`scores[t].argmax(-1)` can name another token than `sequences[:, P + t]`.  The `-inf` pattern does not depend on the logits except
through the timestamp mass rule (timestamps together against the best text token).

`score_sequences` takes the `ops` of the model's engine and calls its `score_tokens`; there is no torch path here.
"""
import torch

from .decoding import rule_kwargs, token_mask


class StepScores(tuple):
    """What `GenerateOutput.scores` / `.logits` hold: a tuple with one fp32 [batch, vocab] tensor per generated step, as the
    reference returns it, that also carries what the kernel computed for the tokens of `sequences`:
    `.tokens` int64 [batch, steps], `.chosen` f32 [batch, steps] (each token's entry of its step's tensor) and `.logprob`
    f32 [batch, steps] (log_softmax of the step's tensor at the token; -inf when a rule masks it).
    A `generate` call that yields no new token gives the empty tuple, as the reference does (the three tensors are then None).

    Unlike the reference's, the step tensors are VIEWS of the one [steps, batch, vocab rounded up to 4] buffer the kernel wrote
    (16-byte stores need rows that start on a multiple of four columns).  When the vocabulary is no multiple of 4 (51 866: row
    stride 51 868) a step tensor is therefore not contiguous -- `.view(-1)` raises where `.reshape(-1)` works --, and each one
    keeps the whole buffer alive; `scores[t].contiguous()` / `.clone()` gives a tensor of its own.  Copying every step here
    would double the feature's memory traffic (up to about 3 GB per call) for callers who never need it."""

    def __new__(cls, steps, tokens=None, chosen=None, logprob=None):
        self = super().__new__(cls, steps)
        self.tokens, self.chosen, self.logprob = tokens, chosen, logprob
        return self


def score_sequences(model, sequences, enc_out, P, rules, want_scores=True, want_logits=False):
    """-> (scores, logits): StepScores or None each.  sequences int64 [B, T] as `generate` produced them (decoder prompt of P
    tokens + generated tokens, finished rows' padding included -- the reference feeds the pad tokens too and scores those steps
    like any other); enc_out: the encoder output the sequences were decoded from; rules: dict(suppress_tokens,
    begin_suppress_tokens, min_new_tokens, eos_token_id, timestamp_rules) as the token loop got them (timestamp_rules: None or
    dict(no_timestamps_token_id, max_initial_timestamp_index))."""
    eng = model.engine
    ops, V = eng.ops, eng.dims.vocab
    B, T = sequences.shape
    L = T - P
    if P < 1 or L < 0:
        raise ValueError(f"sequences of length {T} against a decoder prompt of {P} tokens")
    if L == 0:                                     # no new token (max_new_tokens=0): empty tuples, as the reference returns
        return (StepScores(()) if want_scores else None), (StepScores(()) if want_logits else None)
    seqs = sequences.contiguous()
    logits, _ = eng.decode(seqs[:, :T - 1].contiguous(), enc_out, save=False)       # rows b * (T - 1) + position
    rows = logits[P - 1:]                          # row b * (T - 1) + j predicts sequences[b, P + j]
    gen = seqs[:, P:]

    def run(**kw):
        sc, chosen, logprob = ops.score_tokens(rows, V, seqs, P, L, batch_rows=T - 1, **kw)
        return StepScores(tuple(sc[j] for j in range(L)), gen, chosen, logprob)

    scores = raw = None
    if want_scores:
        eos = rules.get("eos_token_id")
        rk = rule_kwargs(rules.get("timestamp_rules"), eos)
        del rk["begin_index"]                      # (the prompt length: `score_tokens` has it as P)
        scores = run(suppress=token_mask(rules.get("suppress_tokens"), V, seqs.device, torch.uint8),
                     begin_suppress=token_mask(rules.get("begin_suppress_tokens"), V, seqs.device, torch.uint8),
                     min_new=int(rules.get("min_new_tokens") or 0) if eos is not None else 0, **rk)
    if want_logits:
        raw = run()
    return scores, raw


def compute_transition_scores(sequences, scores, beam_indices=None, normalize_logits=False):
    """`GenerationMixin.compute_transition_scores` (TF:generation/utils.py) without beams -> f32 [batch, steps]: the entry of each
    step's tensor at the token `sequences` holds for that step (the last `len(scores)` columns), of the log_softmax of the step's
    tensor with normalize_logits.  For a tuple made by `score_sequences` and the sequences it was made from these are the
    kernel's `chosen` / `logprob`; for anything else the reference's gather in torch."""
    if beam_indices is not None:
        raise NotImplementedError("compute_transition_scores(beam_indices=...) -- scores under beam search -- is not implemented "
                                  "on the MI355X path")
    n = len(scores)
    if n == 0 or sequences.shape[1] < n:
        raise ValueError(f"{n} steps of scores for sequences of length {sequences.shape[1]}")
    idx = sequences[:, sequences.shape[1] - n:]
    if isinstance(scores, StepScores) and scores.chosen is not None and scores.tokens.shape == idx.shape and \
            torch.equal(scores.tokens.to(idx.device), idx):
        return (scores.logprob if normalize_logits else scores.chosen).clone()
    st = torch.stack(tuple(scores), 1).float()                 # [B, steps, V]
    if normalize_logits:
        st = torch.log_softmax(st, dim=-1)
    return st.gather(2, idx.to(st.device)[:, :, None])[:, :, 0]
