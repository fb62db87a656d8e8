"""Token-level timestamps: host side of `WhisperGenerationMixin._extract_token_timestamps` (TF:generation_whisper.py:241-381;
`TF:` = transformers/models/whisper of the pinned transformers 5.15.0) for `generate(return_token_timestamps=True)`.

The reference collects the cross-attention matrix of every decoding step (eager attention, `output_attentions`), copies
[batch, heads, tokens, 1500] to the host and runs `_dynamic_time_warping` (TF:64-115), a double Python loop, per batch row.
Here one teacher-forced decoder pass over the finished sequences (engine.alignment_probs -- the way the original Whisper code
computes it; the same function of the same token prefix) writes the alignment heads' probabilities, and normalisation, median
filter, head average, the dynamic programme and its backtrace run as kernels (csrc/align.hip).  The host sees one int32 per
token: the frame at which the path first reaches it.

Every function takes the `ops` of the model's engine and calls its three alignment methods; there is no torch path here.
"""
import logging

import numpy as np
import torch

logger = logging.getLogger(__name__)
_warned = set()


def warn_once(text):
    """`logger.warning_once` of the reference."""
    if text not in _warned:
        _warned.add(text)
        logger.warning(text)


class TokenTimestampsUnavailable(NotImplementedError, ValueError):
    """`generate(return_token_timestamps=True)` on a generation config without `alignment_heads`.  The reference raises
    ValueError with this text (TF:1689-1693) and callers written against it catch that; this package raised
    NotImplementedError for the whole argument before it had the feature, and callers written against the package caught
    that.  One class derived from both keeps either kind of caller working."""


NO_ALIGNMENT_HEADS = (
    "Model generation config has no `alignment_heads`, token-level timestamps not available. "
    "See https://gist.github.com/hollance/42e32852f24243b748ae6bc1f985b13a on how to add this property to the generation config.")
NO_ATTENTION_MASK = (
    "When setting `return_token_timestamps` to `True`, make sure to pass an `attention_mask` to get precise token-level "
    "timestamps. You can retrieve the `attention_mask` by doing `processor(audio, ..., return_attention_mask=True)` ")
TRANSLATE_WARNING = "Token-level timestamps may not be reliable for task 'translate'."


def check_filter_width(width):
    """TF:49-50."""
    if width <= 0 or width % 2 != 1:
        raise ValueError("`filter_width` should be an odd number")
    if width > 9:
        raise NotImplementedError("median_filter_width above 9 is not implemented on the MI355X path (every Whisper config: 7)")


def frames_per_row(num_frames, batch, max_src):
    """The crop of TF:310-329 / 354 as one frame count per batch row: `num_frames // 2` (mel frames -> encoder positions; a
    slice, so never more than max_src), max_src when no attention mask was given.  A row left with fewer than two mel frames
    has no columns: the reference's DTW then walks its border column and every token of the row gets -1 x time_precision
    (-0.02 s); dw_dtw writes -1 for such a row, the same result (tests/test_token_timestamps.py pins it against `transformers`)."""
    if num_frames is None:
        return [max_src] * batch
    if isinstance(num_frames, (int, np.integer)):
        vals = [int(num_frames)] * batch
    else:
        vals = [int(x) for x in (num_frames.tolist() if hasattr(num_frames, "tolist") else num_frames)]
        if len(vals) != batch:          # (TF:326-329 repeats entries per returned sequence: beams / num_return_sequences, refused here)
            raise ValueError(f"num_frames has {len(vals)} entries for a batch of {batch}")
    return [min(max(v // 2, 0), max_src) for v in vals]


def extract_token_timestamps(model, sequences, enc_out, alignment_heads, num_frames=None, num_input_ids=None,
                             time_precision=0.02, return_intermediates=False):
    """-> float32 [B, seq_len] on `sequences.device`: zeros for the `num_input_ids` prompt positions, the
    time of the first frame the DTW path spends on each generated token, the last value repeated once (the reference has no
    attention row for the last token of a sequence and repeats its predecessor's time, TF:371-379).
    sequences: int64 [B, seq_len] as `generate` produced them (prompt + generated, finished rows' padding included);
    enc_out: the encoder output the sequences were decoded from.  With return_intermediates also (probs, cost, first_frame,
    n_tok, n_frames): the alignment heads' probabilities [B, heads, seq_len - 1, ldp], the DTW cost [B, seq_len - 1, ldc]
    (rows 0 .. n_tok - 1 x columns 0 .. n_frames[b] - 1 valid) and the path's first frame per token."""
    eng = model.engine
    ops, d = eng.ops, eng.dims
    B, T = sequences.shape
    P = int(num_input_ids or 0)
    L = T - 1                                  # positions with an attention row: all but the last token
    width = int(d.median_filter_width)
    check_filter_width(width)
    out = torch.zeros((B, T), dtype=torch.float32, device=sequences.device)
    n_tok = L - P
    if n_tok <= 0:                             # TF:336-339
        return (out, None, None, None, 0, None) if return_intermediates else out
    S = d.max_src
    frames = frames_per_row(num_frames, B, S)
    probs = eng.alignment_probs(sequences[:, :L].contiguous(), enc_out, alignment_heads)
    n_tok_t = torch.full((B,), n_tok, dtype=torch.int32, device=probs.device)
    n_frames_t = torch.tensor(frames, dtype=torch.int32, device=probs.device)
    cost = ops.align_prepare(probs, n_tok_t, n_frames_t, P, S, width)
    first = ops.dtw(cost, n_tok_t, n_frames_t, S)
    ff = first[:, :n_tok].cpu().numpy()
    # TF:369: an integer frame index times a Python float, in double; the float32 result tensor rounds it once
    jump_times = ff.astype(np.int64) * time_precision
    host = np.zeros((B, T), dtype=np.float32)
    host[:, P:P + n_tok] = jump_times
    host[:, P + n_tok] = jump_times[:, -1]
    out = torch.from_numpy(host).to(sequences.device)
    if return_intermediates:
        return out, probs, cost, first, n_tok, frames
    return out
