"""TEST INFRASTRUCTURE -- torch / numpy restatement of the three alignment entry points of libdwamd.so (csrc/align.hip) with the
interface of HipOps, for tests/test_token_timestamps*.py: a subclass of oracle.ref_ops.RefOps that adds them, the reference's
expressions for each stage, and the fixture's scenario plumbing.  The product never imports this module."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import gen_golden_decode as gd
from oracle.ref_ops import RefOps

GOLD_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "token_timestamps.json")


def gold():
    with open(GOLD_PATH) as f:
        return json.load(f)


# ---- stage 1: probabilities (TF:modeling_whisper.py:215-238 eager attention: softmax of q k^T in fp32) -----------------------
def probs_ref(q, k, heads, B, L, Lk, kv_batch_rows, scale=0.125, dtype=torch.float32):
    """q [>= B*L, H*64], k [>= B*kv_batch_rows, H*64] -> [B, len(heads), L, Lk]"""
    out = torch.empty((B, len(heads), L, Lk), dtype=dtype, device=q.device)
    for b in range(B):
        for i, h in enumerate(heads):
            qq = q[b * L:(b + 1) * L, h * 64:(h + 1) * 64].to(dtype) * scale
            kk = k[b * kv_batch_rows:b * kv_batch_rows + Lk, h * 64:(h + 1) * 64].to(dtype)
            out[b, i] = torch.softmax(qq @ kk.t(), -1)
    return out


# ---- stage 2: TF:generation_whisper.py:43-61 and 341-365, expression for expression -----------------------------------------
def median_filter_ref(inputs, filter_width):
    if filter_width <= 0 or filter_width % 2 != 1:
        raise ValueError("`filter_width` should be an odd number")
    pad_width = filter_width // 2
    if inputs.shape[-1] <= pad_width:
        return inputs
    inputs = F.pad(inputs, (pad_width, pad_width, 0, 0), mode="reflect")
    return inputs.unfold(-1, filter_width, 1).sort()[0][..., pad_width]


def prepare_ref(weights, width):
    """weights [heads, tokens, frames] of one batch row (already cropped) -> cost [tokens, frames] = -matrix"""
    std = torch.std(weights, dim=-2, keepdim=True, unbiased=False)
    mean = torch.mean(weights, dim=-2, keepdim=True)
    m = (weights - mean) / std
    m = median_filter_ref(m, width)
    return -m.mean(dim=0)


# ---- stage 3: TF:generation_whisper.py:64-115 walked along anti-diagonals, and the jump extraction of :367-369 ---------------
def dtw_first_frame_ref(matrix):
    """matrix: numpy [N, M] (the cost the reference hands to `_dynamic_time_warping`) -> int64 [N]: time_indices[jumps]."""
    N, M = matrix.shape
    m32 = matrix.astype(np.float32)          # (the reference adds a float64 holding an fp32 value to a float32: one fp32 add)
    cost = np.full((N + 1, M + 1), np.inf, dtype=np.float32)
    trace = np.full((N + 1, M + 1), -1, dtype=np.int8)
    cost[0, 0] = 0
    for d in range(2, N + M + 1):
        i = np.arange(max(1, d - M), min(N, d - 1) + 1)
        j = d - i
        c0, c1, c2 = cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1]
        with np.errstate(invalid="ignore"):
            t0 = (c0 < c1) & (c0 < c2)
            t1 = ~t0 & (c1 < c0) & (c1 < c2)
        t = np.where(t0, 0, np.where(t1, 1, 2))
        c = np.where(t0, c0, np.where(t1, c1, c2))
        with np.errstate(invalid="ignore"):
            cost[i, j] = m32[i - 1, j - 1] + c
        trace[i, j] = t
    trace[0, :] = 2
    trace[:, 0] = 1
    i, j = N, M
    text, time = [], []
    while i > 0 or j > 0:
        text.append(i - 1)
        time.append(j - 1)
        if trace[i, j] == 0:
            i -= 1
            j -= 1
        elif trace[i, j] == 1:
            i -= 1
        else:
            j -= 1
    text, time = np.array(text)[::-1], np.array(time)[::-1]
    jumps = np.pad(np.diff(text), (1, 0), constant_values=1).astype(bool)
    return time[jumps]


def reference_first_frame(matrix):
    """The same through the imported `_dynamic_time_warping` when `transformers` is installed, else the restatement."""
    try:
        from transformers.models.whisper.generation_whisper import _dynamic_time_warping
    except ImportError:
        return dtw_first_frame_ref(matrix)
    text, time = _dynamic_time_warping(np.asarray(matrix, dtype=np.float64))
    jumps = np.pad(np.diff(text), (1, 0), constant_values=1).astype(bool)
    return time[jumps]


class AlignRefOps(RefOps):
    """RefOps + the three alignment ops in torch (fp32 when lowp is float32)."""

    def cross_attn_probs(self, q, k, heads, probs, slot0, B, L, Lk, kv_batch_rows=None, scale=0.125):
        rows = Lk if kv_batch_rows is None else int(kv_batch_rows)
        hs = [int(h) for h in heads.tolist()]
        probs[:, slot0:slot0 + len(hs), :, :Lk] = probs_ref(q, k, hs, B, L, Lk, rows, scale)
        return probs

    def align_prepare(self, probs, n_tok, n_frames, first_tok, max_frames, width, cost=None):
        B, n, L, _ = probs.shape
        if cost is None:
            cost = self.empty((B, L, max_frames), torch.float32)
        for b in range(B):
            N, S = int(n_tok[b]), int(n_frames[b])
            if N > 0 and S > 0:
                cost[b, :N, :S] = prepare_ref(probs[b, :, first_tok:first_tok + N, :S], width)
        return cost

    def dtw(self, cost, n_tok, n_frames, max_frames, first_frame=None):
        B, L, _ = cost.shape
        if first_frame is None:
            first_frame = self.zeros((B, L), torch.int32)
        for b in range(B):
            N, S = int(n_tok[b]), int(n_frames[b])
            if N > 0:
                ff = dtw_first_frame_ref(cost[b, :N, :S].cpu().numpy())
                first_frame[b, :N] = torch.from_numpy(ff.astype(np.int32))
        return first_frame


# ---- fixture scenarios ------------------------------------------------------------------------------------------------------
def fields_of(sc, meta):
    f = gd.generation_fields(multilingual=True, suppress=True, timestamps=sc["ts_fields"])
    f["alignment_heads"] = [list(x) for x in meta["alignment_heads"]]
    return f


def inputs_of(sc):
    B, seed = sc["B"], sc["seed"]
    if sc.get("frames"):
        n = -(-sc["frames"] // 3000)
        f = torch.cat([gd.features(seed + 1 + i, B) for i in range(n)], -1)[..., :sc["frames"]].contiguous()
    else:
        f = gd.features(seed + 1, B)
    mask = None
    if sc.get("mask_frames"):
        mask = torch.zeros(B, f.shape[-1], dtype=torch.long)
        for b, n in enumerate(sc["mask_frames"]):
            mask[b, :n] = 1
    return f, mask


def call_kwargs(sc, device="cpu"):
    kw = dict(sc["kwargs"])
    if "prompt_ids" in kw:
        kw["prompt_ids"] = torch.tensor(kw["prompt_ids"], device=device)
    return kw


def dropin(ops, sc, meta):
    from distil_whisper_amd.generation import GenerationConfig
    from distil_whisper_amd.modeling import WhisperForConditionalGeneration
    m = WhisperForConditionalGeneration(gd.CFG_T, ops=ops, state_dict=gd.weights(sc["seed"]), dtype=torch.float32)
    m.generation_config = GenerationConfig.from_any(fields_of(sc, meta))
    return m


def run_dropin(ops, sc, meta, **extra):
    m = dropin(ops, sc, meta)
    f, mask = inputs_of(sc)
    out = m.generate(f.to(ops.device), attention_mask=None if mask is None else mask.to(ops.device),
                     return_token_timestamps=True, **call_kwargs(sc, ops.device), **extra)
    return m, out


# ---- end-to-end figures (tests/test_token_timestamps_gpu.py asserts them, tools/bench_token_timestamps.py records them) ------
def far_tokens(got, want, frame=0.02):
    """(positions more than one frame apart, positions): every position of `token_timestamps` counts"""
    x, y = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert x.shape == y.shape, (x.shape, y.shape)
    return int((np.abs(x - y) > frame * 1.0001).sum()), int(x.size)


def segment_shares(sc, out):
    """A seek-loop scenario whose tokens equal the fixture's: the segments' and the padded top-level timestamps against the fp32
    fixture, with the bounds max(2 x the reference's own bf16 count, one token)."""
    got = [t for s in out["segments"][0] for t in s["token_timestamps"].tolist()]
    want = [t for s in sc["segments"][0] for t in s["token_timestamps"]]
    bf16 = [t for s in sc["segments_bf16_token_timestamps"][0] for t in s]
    far, total = far_tokens(got, want)
    ref_far, _ = far_tokens(bf16, want)
    top_far, top_total = far_tokens(out["token_timestamps"].cpu().tolist(), sc["token_timestamps"])
    return dict(segment_tokens_far=far, segment_tokens=total, segment_tokens_far_ref_bf16=ref_far,
                segment_tokens_allowed=max(2 * ref_far, 1), tokens_far=top_far, tokens=top_total,
                tokens_allowed=max(2 * sc["ref_bf16_share"] * top_total, 1.0))
