"""TEST INFRASTRUCTURE: the SpecAugment draws of csrc/spec_augment.hip restated in numpy / plain Python from their definition
(include/dwamd.h dw_spec_augment), independently of distil_whisper_amd/spec_augment.py; only Philox4x32-10 is shared with the
dropout restatement.  Also a patch that feeds given masks to `transformers`' `_compute_mask_indices`.
"""
import contextlib

import numpy as np

from dropout_restatement import philox4x32_10

SITE_TIME, SITE_FEATURE = 512, 513


def _words(index, site, seed, step):
    """the four output words (Python ints) of the block with counter (index, site, step_lo, step_hi) under key = seed"""
    seed, step = int(seed) & (2**64 - 1), int(step) & (2**64 - 1)
    w = philox4x32_10((index, site, step & 0xFFFFFFFF, step >> 32), (seed & 0xFFFFFFFF, seed >> 32))
    return [int(x) for x in w]


def epsilon(seed, step, site):
    return _words(0, site, seed, step)[0] * 2.0**-32


def span_count(length, axis_len, prob, mask_length, min_masks, eps):
    n = int(prob * length / mask_length + eps)
    n = max(n, min_masks)
    if n * mask_length > axis_len:
        n = axis_len // mask_length
    if length - (mask_length - 1) < n:
        n = max(length - (mask_length - 1), 0)
    return n


def starts(seed, step, site, b, n, M):
    """Floyd's subset algorithm: n distinct elements of [0, M) in draw order; draw w uses word (w & 3) of block
    ((b + 1) << 16) | (w >> 2)"""
    chosen, seen, blocks = [], set(), {}
    for w in range(n):
        idx = ((b + 1) << 16) | (w >> 2)
        if idx not in blocks:
            blocks[idx] = _words(idx, site, seed, step)
        j = M - n + w
        t = (blocks[idx][w & 3] * (j + 1)) >> 32
        s = j if t in seen else t
        seen.add(s)
        chosen.append(s)
    return chosen


def axis_draws(seed, step, site, B, axis_len, lengths, prob, mask_length, min_masks):
    """-> (epsilon, [starts of row b in draw order] or None when max_n == 0)"""
    eps = epsilon(seed, step, site)
    if span_count(axis_len, axis_len, prob, mask_length, min_masks, eps) == 0:
        return eps, None
    rows = []
    for b in range(B):
        length = axis_len if lengths is None else int(lengths[b])
        n = span_count(length, axis_len, prob, mask_length, min_masks, eps)
        rows.append(starts(seed, step, site, b, n, length - (mask_length - 1)))
    return eps, rows


def axis_mask(seed, step, site, B, axis_len, lengths, prob, mask_length, min_masks):
    """bool [B, axis_len], True = zeroed"""
    _, rows = axis_draws(seed, step, site, B, axis_len, lengths, prob, mask_length, min_masks)
    m = np.zeros((B, axis_len), dtype=bool)
    if rows is None:
        return m
    for b, st in enumerate(rows):
        if not st:
            m[b, axis_len - 1] = True
        for s in st:
            m[b, s:min(s + mask_length, axis_len)] = True
    return m


def masks(seed, step, B, n_mels, T, lengths, p):
    """(time mask [B, T], feature mask [B, n_mels]) of one forward; p: the six mask_* parameters; an axis with prob <= 0 is clear"""
    tm, fm = np.zeros((B, T), dtype=bool), np.zeros((B, n_mels), dtype=bool)
    if p["mask_time_prob"] > 0:
        tm = axis_mask(seed, step, SITE_TIME, B, T, lengths, p["mask_time_prob"], p["mask_time_length"], p["mask_time_min_masks"])
    if p["mask_feature_prob"] > 0:
        fm = axis_mask(seed, step, SITE_FEATURE, B, n_mels, None, p["mask_feature_prob"], p["mask_feature_length"],
                       p["mask_feature_min_masks"])
    return tm, fm


def apply(x, tm, fm):
    """numpy features [B, n_mels, T] -> masked copy"""
    y = np.array(x, copy=True)
    y[np.broadcast_to(tm[:, None, :], y.shape)] = 0.0
    y[np.broadcast_to(fm[:, :, None], y.shape)] = 0.0
    return y


@contextlib.contextmanager
def patched_mask_indices(queue):
    """Inside the block `transformers`' `_compute_mask_indices` returns the next mask of `queue` (numpy bool arrays, in call
    order: the time mask, then the feature mask) instead of drawing."""
    from transformers.models.whisper import modeling_whisper as mw
    orig, todo = mw._compute_mask_indices, list(queue)

    def fake(shape, mask_prob, mask_length, attention_mask=None, min_masks=0):
        assert todo, "more mask draws than masks"
        m = todo.pop(0)
        assert tuple(m.shape) == tuple(shape), (m.shape, shape)
        return np.array(m, dtype=bool)

    mw._compute_mask_indices = fake
    try:
        yield todo
    finally:
        mw._compute_mask_indices = orig


# ---- the case matrix of tests/test_spec_augment.py and tests/test_spec_augment_gpu.py -------------------------------------------
STEPS = (0, 1, 2**32 + 1)


def _axis_cases(axis_lens, extra):
    out = []
    for n in axis_lens:
        for mask_length in (1, 10, n):
            for prob in (0.05, 0.5, 1.0):          # 1.0: the axis_len // mask_length clip
                out.append((n, mask_length, prob, 0))
        out += [(n,) + e for e in extra]
    return out


# (axis_len, mask_length, mask_prob, min_masks): min_masks above the computed count, and a probability with max_n == 0
TIME_CASES = _axis_cases((3000, 202), [(10, 0.05, 40), (10, 1e-6, 0)])
FEATURE_CASES = _axis_cases((80, 128), [(10, 0.05, 3), (10, 1e-6, 0)])


def time_lengths(T):
    """a full row, a long one, one start (10 at mask_length 10) and the zero-span rows (9, 5)"""
    return [T, min(T, 1234), 10, 9, 5]
