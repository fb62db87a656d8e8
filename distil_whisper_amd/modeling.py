"""Drop-in module surface of the reference path over the MI355X engine.

The reference scripts touch exactly two `transformers` classes on the hot path:
  * `WhisperFeatureExtractor.__call__(audio, sampling_rate=...) -> .input_features`
    (run_distillation.py:1176,1234; run_eval.py:628-642; TF:feature_extraction_whisper.py:193-346);
  * `WhisperForConditionalGeneration.forward(input_features=, decoder_input_ids=, labels=)` or
    `forward(encoder_outputs=, labels=)` -> `.loss`, `.logits`, `.encoder_last_hidden_state`, followed by
    `loss.backward()` (run_distillation.py:1472-1484, 1609; TF:modeling_whisper.py:994-1099).
The classes below keep those names, argument meanings, parameter names/shapes (HF `state_dict` keys, tied
`proj_out`), `nn.LayerNorm` instance types (the weight-decay grouping of run_distillation.py:1386-1391 depends on
them) and error behaviour, but every tensor operation runs in the HIP kernels through `WhisperEngine`.
Parameters are views into the engine's flat fp32 master buffer, so `optimizer.step()`, `save_pretrained`-style
`state_dict()`, `load_state_dict()` and DistributedDataParallel all work on them unchanged.
"""
import os
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .engine import ParamStore, WhisperDims, WhisperEngine
from .lazy_logits import LazyLogits, LazyState, _CEFn, _FusedFn, lazy_backward
from .student_init import mel_filter_bank, random_state_dict


def _default_ops(device):
    from .ops_hip import HipOps  # raises when the HIP library or the GPU is missing: there is no CPU fallback
    return HipOps(device)


@dataclass
class Seq2SeqLMOutput:
    loss: Optional[torch.Tensor] = None
    logits: Optional[torch.Tensor] = None
    encoder_last_hidden_state: Optional[torch.Tensor] = None
    # handles for the fused loss kernels (not part of the reference surface): the engine's low-precision logits
    # [rows >= B*T, padded vocabulary] behind `.logits`, and the model that produced them
    _logits_lowp: Optional[torch.Tensor] = None
    _model: Optional[object] = None
    _rows: Optional[object] = None      # _RowSel of a forward called with valid_len (rows of _logits_lowp), else None
    _lazy: Optional[object] = None      # lazy_logits.LazyState shared by `.logits`, `.loss` and the engine node's backward


@dataclass
class BaseModelOutput:
    last_hidden_state: torch.Tensor = None

    def __getitem__(self, i):
        return (self.last_hidden_state,)[i]


class BatchFeature(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e


class WhisperFeatureExtractor:
    """Log-mel front end with the call surface of TF:feature_extraction_whisper.py:193-346, computed on the GPU."""

    def __init__(self, feature_size=80, sampling_rate=16000, hop_length=160, chunk_length=30, n_fft=400,
                 padding_value=0.0, ops=None, device="cuda:0"):
        if n_fft != 400 or hop_length != 160:
            raise ValueError("the HIP log-mel kernel implements Whisper's n_fft=400 / hop_length=160")
        self.feature_size, self.sampling_rate = feature_size, sampling_rate
        self.hop_length, self.chunk_length, self.n_fft = hop_length, chunk_length, n_fft
        self.n_samples = chunk_length * sampling_rate
        self.nb_max_frames = self.n_samples // hop_length
        self.padding_value = padding_value
        self.mel_filters = mel_filter_bank(feature_size)  # [201, n_mels] float64, as the reference attribute
        self.ops = ops if ops is not None else _default_ops(device)
        self._filt = torch.tensor(self.mel_filters, dtype=torch.float32, device=self.ops.device).contiguous()

    def __call__(self, raw_speech, truncation=True, pad_to_multiple_of=None, return_tensors=None,
                 return_attention_mask=None, padding="max_length", max_length=None, sampling_rate=None,
                 do_normalize=None, device=None, **kwargs):
        if sampling_rate is not None and sampling_rate != self.sampling_rate:
            raise ValueError(
                f"The model corresponding to this feature extractor: {self.__class__.__name__} was trained using a "
                f"sampling rate of {self.sampling_rate}. Please make sure that the provided `raw_speech` input was "
                f"sampled with {self.sampling_rate} and not {sampling_rate}.")
        if isinstance(raw_speech, (np.ndarray, torch.Tensor)) and getattr(raw_speech, "ndim", 1) == 1:
            raw_speech = [raw_speech]
        n = max_length if max_length else self.n_samples
        if n % self.hop_length:
            raise ValueError("max_length must be a multiple of hop_length")
        batch = torch.full((len(raw_speech), n), float(self.padding_value), dtype=torch.float32)
        mask = torch.zeros((len(raw_speech), n), dtype=torch.int32)
        for i, w in enumerate(raw_speech):
            w = torch.as_tensor(np.asarray(w, dtype=np.float32)).reshape(-1)
            if w.numel() > n:
                if not truncation:
                    raise ValueError("clips longer than max_length need truncation=True (chunk long audio first)")
                w = w[:n]
            batch[i, : w.numel()] = w
            mask[i, : w.numel()] = 1
        feats = self.ops.logmel(batch.to(self.ops.device), self._filt)
        out = BatchFeature()
        if return_tensors == "pt":
            out["input_features"] = feats
        elif return_tensors == "np" or return_tensors is None:
            arr = feats.cpu().numpy()
            out["input_features"] = arr if return_tensors == "np" else [a for a in arr]
        else:
            raise ValueError(f"unsupported return_tensors={return_tensors}")
        if return_attention_mask:
            out["attention_mask"] = mask[:, :: self.hop_length]
        return out


    def pad(self, processed_features, padding=True, max_length=None, truncation=False, pad_to_multiple_of=None,
            return_attention_mask=None, return_tensors=None):
        """`SequenceFeatureExtractor.pad` as the reference's collator calls it (run_distillation.py:447-451:
        `pad({"input_features": [M x 3000 arrays]}, padding="max_length", return_tensors="pt")`).  The base class
        pads along the FIRST axis of every item (the mel-bin axis for Whisper features, which is equal for all items),
        so the call (`padding="longest"` at run_distillation.py:1421) amounts to stacking the already fixed-length features into one float32 batch; items whose first
        axes differ are padded with `padding_value` up to the longest (or `max_length`)."""
        if isinstance(processed_features, (list, tuple)):
            processed_features = {k: [f[k] for f in processed_features] for k in processed_features[0]}
        if "input_features" not in processed_features:
            raise ValueError("You should supply an instance of `BatchFeature` or list of `BatchFeature` to this "
                             f"method that includes input_features, but you provided {list(processed_features.keys())}")
        items = [torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x).to(torch.float32)
                 for x in processed_features["input_features"]]
        out = BatchFeature()
        if len(items) == 0:
            out["input_features"] = []
            return out
        do_pad = padding not in (False, "do_not_pad")
        if padding == "max_length" and max_length is None:
            raise ValueError("When setting ``padding=max_length``, make sure that max_length is defined")
        n0 = max(x.shape[0] for x in items)
        if do_pad and padding == "max_length" and max_length is not None:
            n0 = max_length
        if do_pad and pad_to_multiple_of:
            n0 = -(-n0 // pad_to_multiple_of) * pad_to_multiple_of
        rows, masks = [], []
        for x in items:
            if truncation and max_length is not None and x.shape[0] > max_length:
                x = x[:max_length]
            m = torch.ones(x.shape[0], dtype=torch.int32)
            if do_pad and x.shape[0] < n0:
                fill = torch.full((n0 - x.shape[0],) + tuple(x.shape[1:]), float(self.padding_value))
                x = torch.cat([x, fill], 0)
                m = torch.cat([m, torch.zeros(n0 - m.numel(), dtype=torch.int32)])
            rows.append(x)
            masks.append(m)
        if return_tensors in ("pt", "np"):
            if any(r.shape != rows[0].shape for r in rows):
                raise ValueError("Unable to convert output 'input_features' to tensor: the items have different "
                                 "shapes. Use padding=True to ensure all outputs have the same length.")
            batch = torch.stack(rows)
            out["input_features"] = batch if return_tensors == "pt" else batch.numpy()
            if return_attention_mask:
                am = torch.stack(masks)
                out["attention_mask"] = am if return_tensors == "pt" else am.numpy()
        elif return_tensors is None:
            out["input_features"] = [r.numpy() for r in rows]
            if return_attention_mask:
                out["attention_mask"] = [m.numpy() for m in masks]
        else:
            raise ValueError(f"unsupported return_tensors={return_tensors}")
        return out

    # -- checkpoint directory round trip (run_distillation.py:966, 1071, 1641) ------------------------------------------
    def to_dict(self):
        return {"feature_extractor_type": "WhisperFeatureExtractor", "feature_size": self.feature_size,
                "sampling_rate": self.sampling_rate, "hop_length": self.hop_length, "chunk_length": self.chunk_length,
                "n_fft": self.n_fft, "padding_value": self.padding_value, "n_samples": self.n_samples,
                "nb_max_frames": self.nb_max_frames, "padding_side": "right", "return_attention_mask": False}

    def save_pretrained(self, save_directory, **kwargs):
        import json
        import os
        os.makedirs(save_directory, exist_ok=True)
        with open(os.path.join(save_directory, "preprocessor_config.json"), "w") as f:
            json.dump(self.to_dict(), f, indent=2, sort_keys=True)

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, ops=None, device="cuda:0", **kwargs):
        import json
        import os
        path = os.path.join(str(pretrained_model_name_or_path), "preprocessor_config.json")
        if not os.path.exists(path):
            raise OSError(f"{path} not found (no hub access in this environment: pass a local checkpoint directory)")
        with open(path) as f:
            d = json.load(f)
        keys = ("feature_size", "sampling_rate", "hop_length", "chunk_length", "n_fft", "padding_value")
        return cls(**{k: d[k] for k in keys if k in d}, ops=ops, device=device)


class _EncoderLayer(nn.Module):
    def __init__(self, D, Fd):
        super().__init__()
        self.self_attn = _Attention(D)
        self.self_attn_layer_norm = nn.LayerNorm(D, device="meta")
        self.fc1 = nn.Linear(D, Fd, device="meta")
        self.fc2 = nn.Linear(Fd, D, device="meta")
        self.final_layer_norm = nn.LayerNorm(D, device="meta")


class _DecoderLayer(nn.Module):
    def __init__(self, D, Fd):
        super().__init__()
        self.self_attn = _Attention(D)
        self.self_attn_layer_norm = nn.LayerNorm(D, device="meta")
        self.encoder_attn = _Attention(D)
        self.encoder_attn_layer_norm = nn.LayerNorm(D, device="meta")
        self.fc1 = nn.Linear(D, Fd, device="meta")
        self.fc2 = nn.Linear(Fd, D, device="meta")
        self.final_layer_norm = nn.LayerNorm(D, device="meta")


class _Attention(nn.Module):
    def __init__(self, D):
        super().__init__()
        self.k_proj = nn.Linear(D, D, bias=False, device="meta")
        self.v_proj = nn.Linear(D, D, device="meta")
        self.q_proj = nn.Linear(D, D, device="meta")
        self.out_proj = nn.Linear(D, D, device="meta")


class _Encoder(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.conv1 = nn.Conv1d(d.n_mels, d.d_model, 3, padding=1, device="meta")
        self.conv2 = nn.Conv1d(d.d_model, d.d_model, 3, stride=2, padding=1, device="meta")
        self.embed_positions = nn.Embedding(d.max_src, d.d_model, device="meta")
        self.layers = nn.ModuleList([_EncoderLayer(d.d_model, d.ffn) for _ in range(d.enc_layers)])
        self.layer_norm = nn.LayerNorm(d.d_model, device="meta")
        self.gradient_checkpointing = False     # read by run_distillation.py:1021 / 1037 before anyone enables it


class _Decoder(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.embed_tokens = nn.Embedding(d.vocab, d.d_model, device="meta")
        self.embed_positions = nn.Embedding(d.max_tgt, d.d_model, device="meta")
        self.layers = nn.ModuleList([_DecoderLayer(d.d_model, d.ffn) for _ in range(d.dec_layers)])
        self.layer_norm = nn.LayerNorm(d.d_model, device="meta")
        self.gradient_checkpointing = False


class _Model(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.encoder = _Encoder(d)
        self.decoder = _Decoder(d)


def check_regularisers(config):
    """`dropout` and `activation_dropout` (the row-local dropouts: embeddings, the three residual branches, the GELU output of
    fc1) and SpecAugment (`apply_spec_augment`, spec_augment.py) are built and apply in training mode; the other regularisers
    of `transformers.WhisperConfig` are not."""
    from .spec_augment import params_from_config, validate
    sa = params_from_config(config)
    if sa is not None:      # the reference's messages, at construction instead of the first training forward
        validate(sa, int(getattr(config, "num_mel_bins", 80)), 2 * int(getattr(config, "max_source_positions", 1500)))
    for k in ("dropout", "activation_dropout"):
        v = getattr(config, k, 0.0) or 0.0
        if not 0.0 <= float(v) < 1.0:
            raise ValueError(f"{k}={v}: a probability in [0, 1) is expected")
    bad = [k for k in ("attention_dropout", "encoder_layerdrop", "decoder_layerdrop") if getattr(config, k, 0.0)]
    if getattr(config, "scale_embedding", False):
        bad.append("scale_embedding")
    if bad:
        raise ValueError(f"{', '.join(bad)}: not implemented on the MI355X path, which builds `dropout` and `activation_dropout` "
                         "only (attention_dropout needs the mask inside the flash-attention kernels, layerdrop changes the "
                         "launch sequence of a captured step; scale_embedding is False in every Whisper config)")


class WhisperConfig:
    """The fields of `transformers.WhisperConfig` this path reads (TF:configuration_whisper.py:127-164), loadable from
    and writable to a checkpoint directory's config.json.  A `transformers.WhisperConfig` works in its place."""

    model_type = "whisper"
    _DEFAULTS = dict(vocab_size=51865, num_mel_bins=80, encoder_layers=4, encoder_attention_heads=6, decoder_layers=4,
                     decoder_attention_heads=6, decoder_ffn_dim=1536, encoder_ffn_dim=1536, d_model=384,
                     max_source_positions=1500, max_target_positions=448, pad_token_id=50256, bos_token_id=50256,
                     eos_token_id=50256, decoder_start_token_id=50257, activation_function="gelu", dropout=0.0,
                     attention_dropout=0.0, activation_dropout=0.0, encoder_layerdrop=0.0, decoder_layerdrop=0.0,
                     scale_embedding=False, use_cache=True, suppress_tokens=None, begin_suppress_tokens=None,
                     max_length=448, forced_decoder_ids=None, apply_spec_augment=False, mask_time_prob=0.05,
                     mask_time_length=10, mask_time_min_masks=2, mask_feature_prob=0.0, mask_feature_length=10,
                     mask_feature_min_masks=0)

    def __init__(self, **kw):
        for k, v in self._DEFAULTS.items():
            setattr(self, k, v)
        for k, v in kw.items():
            setattr(self, k, v)
        if self.encoder_attention_heads != self.decoder_attention_heads or self.encoder_ffn_dim != self.decoder_ffn_dim:
            raise ValueError("the MI355X engine expects equal encoder / decoder head counts and FFN widths")
        if self.d_model != 64 * self.encoder_attention_heads:
            raise ValueError("the HIP attention kernel implements head_dim 64 (every Whisper checkpoint)")
        if self.activation_function != "gelu":
            raise ValueError("the HIP GEMM epilogue implements Whisper's exact GELU")
        check_regularisers(self)

    def to_dict(self):
        d = {k: v for k, v in vars(self).items() if not k.startswith("_")}
        d["model_type"] = "whisper"
        d["architectures"] = ["WhisperForConditionalGeneration"]
        return d

    @classmethod
    def from_pretrained(cls, path, **_):
        import json
        import os
        with open(os.path.join(path, "config.json")) as f:
            d = json.load(f)
        for k in ("model_type", "architectures", "transformers_version", "torch_dtype", "dtype", "_name_or_path"):
            d.pop(k, None)
        return cls(**d)

    def save_pretrained(self, path):
        import json
        import os
        os.makedirs(path, exist_ok=True)
        with open(os.path.join(path, "config.json"), "w") as f:
            json.dump(self.to_dict(), f, indent=2, sort_keys=True)


class _RowSel:
    """Which decoder positions a forward computed when it was told the label lengths (`valid_len`, see
    distill.trim_dead_positions): the first `Te` positions of every sequence, or -- per-sequence lengths -- the packed live
    rows (engine.LiveRows over the [B, Te] rectangle).  The engine's low-precision logits hold exactly these rows; the
    reference-shaped fp32 `.logits` [B, T, V] keeps its shape with ZERO rows at the dead positions (labels -100 there:
    the reference's CE ignores them and its KL term masks them, run_distillation.py:1453-1462)."""

    def __init__(self, B, T, Te, live):
        self.B, self.T, self.Te, self.live = B, T, Te, live
        self.n = B * Te if live is None else live.n
        self.idx_full = None
        if live is not None:
            i = live.idx.long()
            self.idx_full = (i // Te) * T + i % Te          # row numbers in the full [B * T] layout

    @classmethod
    def make(cls, valid_len, B, T, device, pack_below=0.9):
        from .distill import _as_int
        from .engine import LiveRows
        valid_len = _as_int(valid_len)
        if valid_len is None:
            return None
        lens = None
        if not isinstance(valid_len, int):
            lens = [max(1, min(T, int(x))) for x in valid_len]
            if len(lens) != B:
                raise ValueError("valid_len: one length per sequence of the batch (or one int for the batch)")
            valid_len = max(lens)
        Te = max(1, min(T, int(valid_len)))
        live = None
        if lens is not None and sum(lens) < pack_below * B * Te:
            live = LiveRows.build(lens, Te, device)
        if Te == T and live is None:
            return None
        return cls(B, T, Te, live)

    def same_as(self, other):
        if other is None or (self.B, self.T, self.Te, self.n) != (other.B, other.T, other.Te, other.n):
            return False
        return (self.live is None) == (other.live is None) and (self.live is None or torch.equal(self.live.idx, other.live.idx))

    def select(self, flat):
        """[B * T, C] in (batch, position) order -> the computed rows [n, C]"""
        if self.live is None:
            return flat.reshape(self.B, self.T, -1)[:, :self.Te].reshape(self.B * self.Te, -1)
        return flat.index_select(0, self.idx_full)

    def expand(self, rows, V):
        """computed rows [n, >= V] -> fp32 [B, T, V], zeros at the positions that were not computed"""
        B, T, Te = self.B, self.T, self.Te
        out = torch.zeros(B, T, V, dtype=torch.float32, device=rows.device)
        if self.live is None:
            out[:, :Te] = rows[: B * Te, :V].reshape(B, Te, V)
        else:
            out.view(B * T, V).index_copy_(0, self.idx_full, rows[: self.n, :V].float())
        return out


class _PendingLens:
    """The label lengths of a batch on their way to the host (`WhisperForConditionalGeneration.skip_dead_positions`).

    The reference hands the model `labels` padded to 448 with -100 (run_distillation.py:405-478) and computes all 447
    decoder positions of every row; positions behind a row's last label are dead (distill.trim_dead_positions: same loss,
    same gradients without them -- 71 % of the benchmark's decoder positions).  Leaving them out needs the lengths ON THE
    HOST (they size the launches), and the drop-in collator can put them into the batch (`report_valid_len`) -- but that is
    an edit of the script.  Without it the lengths are read back from the device tensor the model is given: a tiny reduction
    and a non-blocking copy into pinned memory are enqueued FIRST, the whole encoder forward (which does not depend on them)
    is enqueued next, and only then the host waits for the copy's event -- by which time the device has >= 100 ms of encoder
    work queued, so the wait costs the host its run-ahead over the previous step and the device nothing.  The second model
    called with the same `labels` tensor (the teacher: `teacher_model(**batch)` / `(encoder_outputs=..., labels=...)`) finds
    the lengths in a one-entry cache keyed by the tensor's address, shape and version: no second round trip."""

    _cache = {}

    def __init__(self, labels):
        self.key = (labels.data_ptr(), tuple(labels.shape), labels._version, str(labels.device))
        self.lens = _PendingLens._cache.get(self.key)
        self.event = None
        if self.lens is None:
            T = labels.shape[1]
            pos = torch.arange(1, T + 1, device=labels.device)
            lens_dev = ((labels != -100) * pos).amax(dim=1)
            if labels.is_cuda:
                self.host = torch.empty(labels.shape[0], dtype=torch.int64, pin_memory=True)
                self.host.copy_(lens_dev, non_blocking=True)
                self.event = torch.cuda.Event()
                self.event.record()
            else:
                self.host = lens_dev

    def resolve(self):
        if self.lens is None:
            if self.event is not None:
                self.event.synchronize()
            self.lens = [max(1, int(x)) for x in self.host.tolist()]
            _PendingLens._cache.clear()
            _PendingLens._cache[self.key] = self.lens
        return self.lens


class _EngineFn(torch.autograd.Function):
    """forward: engine encode+decode with activations kept; backward: engine backward from d(loss)/d(logits) (and
    optionally d/d(encoder_last_hidden_state)); parameter gradients are returned as views of the flat buffer."""

    @staticmethod
    def forward(ctx, model, input_features, enc_in, decoder_input_ids, sel, *params):
        eng = model.engine
        train = any(ctx.needs_input_grad[5:])  # (grad mode is off inside Function.forward; this is the real signal)
        enc_train = train and model._encoder_requires_grad()
        ectx = None
        eng.training = bool(train and model.training)
        # SpecAugment masks on the module's training flag alone, in front of the encoder (so not when `encoder_outputs` came
        # in), and in place on the caller's tensor -- TF:modeling_whisper.py WhisperModel.forward / _mask_input_features
        augment = bool(model.training and eng.spec is not None and enc_in is None)
        lengths, model._spec_lengths = model._spec_lengths, None
        if eng.training or augment:
            eng.dropout_tick()          # this forward draws the masks of the next step (nothing happens with everything off)
        if augment:
            if input_features.dtype == torch.float32 and input_features.is_contiguous():
                eng.spec_augment(input_features, lengths=lengths)
            else:
                masked = eng.spec_augment(input_features.to(torch.float32).contiguous(), lengths=lengths)
                input_features.copy_(masked)
                input_features = masked
        if enc_in is None:
            enc, ectx = eng.encode(input_features.to(torch.float32).contiguous(), save=enc_train)
        else:
            rows = enc_in.shape[0] * enc_in.shape[1]
            enc = eng.act(rows, eng.dims.d_model)
            enc[:rows].copy_(enc_in.reshape(rows, -1))
        B, T = decoder_input_ids.shape
        V = eng.dims.vocab
        if isinstance(sel, _PendingLens):       # label lengths read back from the device: the encoder is queued, now wait
            sel = _RowSel.make(sel.resolve(), B, T, decoder_input_ids.device)
        model._last_sel = sel
        if sel is None:
            logits, dctx = eng.decode(decoder_input_ids.contiguous(), enc, save=train)
        else:
            # the dead decoder positions are left out (same loss, same gradients: distill.trim_dead_positions)
            logits, dctx = eng.decode(decoder_input_ids[:, :sel.Te].contiguous(), enc, save=train, live=sel.live)
        # `.logits` keeps the reference's type and shape -- fp32 [B, T, V], accelerate upcasts model outputs to fp32 -- but the
        # allocation is left UNFILLED: the values stay in the engine's bf16 buffer until something other than the reference's
        # own loss expression reads them (lazy_logits.LazyLogits; the wrapper is put on by `forward`, which owns the state)
        out_logits = torch.empty((B, T, V), dtype=torch.float32, device=logits.device)
        state = LazyState(model, logits, sel, (B, T, V), train)
        ctx.set_materialize_grads(False)
        ctx.model, ctx.ectx, ctx.dctx, ctx.shape, ctx.sel = model, ectx, dctx, (B, T, V), sel
        ctx.logits_buf = logits if train else None
        ctx.lazy = state
        model._last_logits_lowp = logits
        model._last_lazy_state = state
        Re = B * eng.dims.max_src
        enc_out = enc[:Re].float().view(B, eng.dims.max_src, -1)
        ctx.mark_non_differentiable(enc_out)
        return out_logits, enc_out

    @staticmethod
    def backward(ctx, g_logits, _g_enc):
        model, eng = ctx.model, ctx.model.engine
        B, T, V = ctx.shape
        st = eng.st
        buf = ctx.logits_buf
        if not lazy_backward(ctx.lazy, buf, g_logits):
            # no loss node left its upstream gradient behind: the caller differentiated through the materialised tensor
            buf.zero_()
            if g_logits is not None:
                if ctx.sel is None:
                    buf[: B * T, :V].copy_(g_logits.reshape(B * T, V))
                else:
                    buf[: ctx.sel.n, :V].copy_(ctx.sel.select(g_logits.reshape(B * T, V)))
        # (the flat buffer is this backward's scratch: cleared here, so the layers' weight gradients are stored, not added)
        # (not when this backward stops at `encoder_outputs` while the encoder is trainable: its weight gradients must read zero)
        every_weight_written = ctx.ectx is not None or not st.is_trainable("model.encoder.layers.0.fc1.weight")
        eng.zero_small_grads(skip_weights=every_weight_written)
        eng.wgrad_overwrite = True
        try:
            denc = eng.backward_decoder(ctx.dctx, buf, want_denc=ctx.ectx is not None)
            if ctx.ectx is not None:
                eng.backward_encoder(ctx.ectx, denc)
        finally:
            eng.wgrad_overwrite = False
        # copies of the flat gradient buffer's ranges: the buffer is zeroed and rewritten by the next backward, so a
        # returned view would change under torch.autograd.grad results, tensor hooks or DDP bucket views that keep it.
        # (AccumulateGrad takes ownership of a fresh non-view gradient without copying it again: still one copy.)
        # Parameters frozen after construction (`requires_grad_(False)`, run_distillation.py:1018-1040) get None.
        # ONE copy of the trainable range (a single launch, not ~600 five-microsecond ones on a host that is the bottleneck of the
        # eager loop); every returned gradient is a contiguous view of that fresh buffer, which nothing else writes.
        lo, hi = st.train_start, st.train_end
        Gc = st.G[lo:hi].clone() if hi > lo else None
        grads = []
        for name, p in zip(model._param_names, model._param_list):
            if p.requires_grad and name in st.g:
                off = st.entries[name][0]
                grads.append(Gc[off - lo: off - lo + p.numel()].view(p.shape))
            else:
                grads.append(None)
        return (None, None, None, None, None, *grads)


def fused_distillation_loss(student_outputs, teacher_outputs, labels, temperature=2.0, kl_weight=1.0, ce_weight=0.8):
    """One-call replacement for lines 1486-1493 of run_distillation.py (`ce_loss`, the two softmaxes, `kl_divergence`,
    `loss = 0.8 * ce_loss + kl_weight * kl_loss`) when both models are `distil_whisper_amd` modules: the fused HIP loss
    kernel reads the two engines' bf16 logits once.  Returns (loss, {"loss", "ce_loss", "kl_loss"}) with the metrics
    detached, like the reference's `metrics` dict (1494-1495).  `loss.backward()` then runs the student's backward."""
    s_buf, t_buf = student_outputs._logits_lowp, teacher_outputs._logits_lowp
    if s_buf is None or t_buf is None:
        raise ValueError("fused_distillation_loss needs outputs of distil_whisper_amd.WhisperForConditionalGeneration")
    model = student_outputs._model
    sel = student_outputs._rows
    t_sel = teacher_outputs._rows
    if sel is not None and t_sel is None:
        # The reference's shared-encoder call `teacher_model(encoder_outputs=..., labels=...)` (run_distillation.py:1478)
        # carries no `valid_len`: the teacher computed all B * T rows.  Take the student's rows out of them (a row gather of
        # the teacher's low-precision logits: B * Te * V * 2 B of traffic, against a step-0 ValueError before).
        BT = sel.B * sel.T
        if t_buf.shape[0] < BT:
            raise ValueError("fused_distillation_loss: the teacher's logits do not cover the student's batch")
        t_buf = sel.select(t_buf[:BT]).contiguous()
    elif (sel is None) != (t_sel is None) or (sel is not None and not sel.same_as(t_sel)):
        raise ValueError("fused_distillation_loss: student and teacher outputs were computed over different decoder "
                         "positions (pass the same valid_len to both forwards, or none to the teacher)")
    state = student_outputs._lazy
    B, T = labels.shape
    R = state.rows
    lab = state.select_rows(labels.reshape(B * T, 1)).reshape(-1).contiguous()
    t_rows = t_buf[:R]
    loss, losses = _FusedFn.apply(student_outputs.logits.as_subclass(torch.Tensor), state, t_rows, lab, float(temperature),
                                  float(ce_weight), float(kl_weight))
    return loss, {"loss": losses[2], "ce_loss": losses[0], "kl_loss": losses[1]}


def _assistant_shares_encoder(assistant_model, d):
    """True: the assistant of speculative decoding drafts on the target's encoder output -- a full model whose owner set
    `share_encoder_output`, or a decoder-only `WhisperForCausalLM`, which has no encoder of its own (TF hands the target's
    `encoder_outputs` to such an assistant, TF:generation/candidate_generator.py)."""
    if getattr(assistant_model, "decoder_only", False):
        if assistant_model.dims.d_model != d.d_model:
            raise ValueError(f"the decoder-only assistant has d_model = {assistant_model.dims.d_model}, the model it drafts for "
                             f"has d_model = {d.d_model}: a WhisperForCausalLM assistant cross-attends to the target's encoder "
                             "output and needs the same d_model")
        return True
    return bool(getattr(assistant_model, "share_encoder_output", None))


class WhisperForConditionalGeneration(nn.Module):
    """dtype=torch.float32 (default): fp32 master weights, bf16 GEMM operands, fp32 residual stream -- the reference's
    student under `accelerate` bf16 autocast (SURVEY.md section 8a').  dtype=torch.bfloat16: weights rounded to bf16
    and a bf16 residual stream -- a model loaded with `torch_dtype=torch.bfloat16` (the teacher of
    run_distillation.py:986-1004, every model of run_eval.py / run_pseudo_labelling.py); inference only."""

    # `forward(..., labels=...)` without `valid_len`: read the label lengths back from `labels` and leave the dead decoder
    # positions out (_PendingLens).  Same loss and gradients under the reference's loss lines (CE ignores -100, the KL term is
    # masked by labels >= 0); `.logits` then has ZERO rows behind each row's last label, which a caller that looks at padded
    # positions would see -- so it is OFF unless asked for: `DW_SKIP_DEAD_POSITIONS=1` in the environment of the unedited
    # script, or `model.skip_dead_positions = True`.
    skip_dead_positions = os.environ.get("DW_SKIP_DEAD_POSITIONS", "0") not in ("", "0", "false", "False")

    def __init__(self, config, ops=None, device="cuda:0", state_dict=None, seed=0, frozen_prefixes=(),
                 dtype=torch.float32, dropout_seed=0):
        super().__init__()
        check_regularisers(config)
        self.config = config
        self.dims = WhisperDims.from_any(config)
        self.ops = ops if ops is not None else _default_ops(device)
        if dtype not in (torch.float32, torch.bfloat16, None):
            raise ValueError(f"dtype {dtype}: the MI355X path computes in bf16 with fp32 or bf16 parameters")
        self.dtype_mode = torch.float32 if dtype is None else dtype
        pure_bf16 = self.dtype_mode == torch.bfloat16
        sd = state_dict if state_dict is not None else random_state_dict(self.dims, seed, device=self.ops.device)
        self.store = ParamStore(self.ops, self.dims, sd, trainable=not pure_bf16,
                                frozen_prefixes=tuple(frozen_prefixes), round_bf16=pure_bf16)
        self.engine = WhisperEngine(self.ops, self.store, self.ops.lowp if pure_bf16 else torch.float32)
        # `config.dropout` / `config.activation_dropout` apply to training-mode forwards that keep activations (module.train(),
        # parameters that require grad), as in the reference's layers; the inference-only bf16 model ignores them
        p_drop, p_act = float(getattr(config, "dropout", 0.0) or 0.0), float(getattr(config, "activation_dropout", 0.0) or 0.0)
        if not pure_bf16 and (p_drop or p_act):
            self.engine.set_dropout(p_drop, p_act, seed=dropout_seed)
        # `config.apply_spec_augment`: training-mode forwards mask the input features in place (spec_augment.py); seed and step
        # counter are dropout's
        from .spec_augment import params_from_config
        if not pure_bf16:
            self.engine.set_spec_augment(params_from_config(config), seed=dropout_seed)
        self._spec_lengths = None
        self._decoders = {}
        self.model = _Model(self.dims)
        self.proj_out = nn.Linear(self.dims.d_model, self.dims.vocab, bias=False, device="meta")
        # re-point every parameter of the (meta) module tree at its view in the flat master buffer
        for name in self.store.real_names():
            mod_path, pname = name.rsplit(".", 1)
            mod = self.get_submodule(mod_path)
            p = nn.Parameter(self.store.p[name], requires_grad=self.store.is_trainable(name))
            setattr(mod, pname, p)
        self.proj_out.weight = self.model.decoder.embed_tokens.weight  # tied (TF:modeling_whisper.py:965)
        self._param_names = self.store.real_names()
        self._param_list = [self.get_parameter(n) for n in self._param_names]
        self._enc_params = [p for n, p in zip(self._param_names, self._param_list) if n.startswith("model.encoder.")]
        self._versions = None
        from .generation import GenerationConfig
        self.generation_config = GenerationConfig.from_model_config(config)
        if self.generation_config.decoder_start_token_id is None:
            self.generation_config.decoder_start_token_id = self.dims.decoder_start_token_id
        self.is_gradient_checkpointing = False

    # -- reference surface ------------------------------------------------------------------------------------------
    def state_dict(self, *args, destination=None, prefix="", keep_vars=False):
        """`nn.Module.state_dict()` with INDEPENDENT tensors.  Every parameter of this module is a view of one flat
        buffer (engine.ParamStore); serializers that look at storages -- safetensors behind `accelerator.save_state`
        (run_distillation.py:1636) -- take tensors that share a storage for aliases of one another, drop all but one and
        then refuse the rest ("None is covering the entire storage").  So the entries are copies, and the tied
        `proj_out.weight` IS `model.decoder.embed_tokens.weight` (one tensor under two names, as `transformers` hands it
        out).  `keep_vars=True` returns the live parameters (views) unchanged."""
        sd = super().state_dict(*args, destination=destination, prefix=prefix, keep_vars=keep_vars)
        if keep_vars:
            return sd
        mine = [k for k in sd if k.startswith(prefix)]
        for k in mine:
            sd[k] = sd[k].clone()
        tied, emb = prefix + "proj_out.weight", prefix + "model.decoder.embed_tokens.weight"
        if tied in sd and emb in sd:
            sd[tied] = sd[emb]
        return sd

    def get_encoder(self):
        return self.model.encoder

    def get_decoder(self):
        return self.model.decoder

    def _encoder_requires_grad(self):
        return any(p.requires_grad for p in self._enc_params)

    def freeze_encoder(self):
        """`student_model.freeze_encoder()` (run_distillation.py:1018-1021; TF:modeling_whisper.py `freeze_encoder` ->
        `encoder._freeze_parameters()`): gradients of the encoder are disabled.  The engine then neither keeps the
        encoder's activations nor runs its backward; the same happens for any parameter the caller switches off with
        `requires_grad_(False)` afterwards (run_distillation.py:1034-1040 `freeze_embed_positions`)."""
        for p in self._enc_params:
            p.requires_grad_(False)
        self.model.encoder._requires_grad = False

    def gradient_checkpointing_enable(self, gradient_checkpointing_kwargs=None):
        """run_distillation.py:1014-1015.  The engine keeps every activation it needs in HBM (288 GB: the full
        distil-large-v3 step at batch 32 peaks at 94 GiB) and never recomputes, so this only records the request."""
        self.is_gradient_checkpointing = True
        self.model.encoder.gradient_checkpointing = True
        self.model.decoder.gradient_checkpointing = True

    def gradient_checkpointing_disable(self):
        self.is_gradient_checkpointing = False
        self.model.encoder.gradient_checkpointing = False
        self.model.decoder.gradient_checkpointing = False

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, *model_args, config=None, torch_dtype=None, dtype=None,
                        attn_implementation=None, low_cpu_mem_usage=None, cache_dir=None, revision=None, token=None,
                        subfolder="", variant=None, use_safetensors=None, local_files_only=None, ops=None,
                        device="cuda:0", **kwargs):
        """Load `config.json` + `model.safetensors` (or `pytorch_model.bin`) from a LOCAL checkpoint directory
        (run_distillation.py:986-1004, run_eval.py:547-563 call this with hub names; there is no network here, so a
        name that is not a directory raises).  `attn_implementation` is accepted for the CLI whitelist
        (run_distillation.py:141-148): this class always runs the HIP flash-attention kernel."""
        import json
        import os
        if kwargs:
            raise TypeError(f"from_pretrained() got unexpected keyword arguments {sorted(kwargs)}")
        path = os.path.join(str(pretrained_model_name_or_path), subfolder) if subfolder else \
            str(pretrained_model_name_or_path)
        if not os.path.isdir(path):
            raise OSError(f"{path} is not a local checkpoint directory (no hub access in this environment)")
        if attn_implementation not in (None, "eager", "sdpa", "flash_attention_2", "hip_attention"):
            raise ValueError(f"unknown attn_implementation {attn_implementation!r}")
        if config is None:
            config = WhisperConfig.from_pretrained(path)
        dt = dtype if dtype is not None else torch_dtype
        if isinstance(dt, str):
            dt = {"float32": torch.float32, "bfloat16": torch.bfloat16, "auto": None}.get(dt, dt)
        st_path = os.path.join(path, "model.safetensors" if not variant else f"model.{variant}.safetensors")
        bin_path = os.path.join(path, "pytorch_model.bin")
        if os.path.exists(st_path) and use_safetensors is not False:
            from safetensors.torch import load_file
            sd = load_file(st_path)
        elif os.path.exists(bin_path):
            sd = torch.load(bin_path, map_location="cpu", weights_only=True)
        else:
            raise OSError(f"no model.safetensors / pytorch_model.bin under {path}")
        if "model.decoder.embed_tokens.weight" not in sd and "proj_out.weight" in sd:
            sd["model.decoder.embed_tokens.weight"] = sd["proj_out.weight"]
        model = cls(config, ops=ops, device=device, state_dict=sd, dtype=dt)
        gpath = os.path.join(path, "generation_config.json")
        if os.path.exists(gpath):
            from .generation import GenerationConfig
            with open(gpath) as f:
                model.generation_config = GenerationConfig.from_any(json.load(f))
        return model

    def save_pretrained(self, save_directory, state_dict=None, safe_serialization=True, **kwargs):
        """run_distillation.py:1765, 1791: config.json, generation_config.json and the weights under their HF names
        (the tied `proj_out.weight` is not stored, as `transformers` does for tied weights)."""
        import json
        import os
        os.makedirs(save_directory, exist_ok=True)
        cfg = self.config
        if hasattr(cfg, "save_pretrained"):
            cfg.save_pretrained(save_directory)
        else:
            WhisperConfig(**{k: getattr(cfg, k) for k in WhisperConfig._DEFAULTS if hasattr(cfg, k)}) \
                .save_pretrained(save_directory)
        with open(os.path.join(save_directory, "generation_config.json"), "w") as f:
            json.dump(self.generation_config.to_dict(), f, indent=2, sort_keys=True)
        sd = state_dict if state_dict is not None else self.state_dict()
        sd = {k: v.detach().to("cpu").contiguous() for k, v in sd.items() if k != "proj_out.weight"}
        if safe_serialization:
            from safetensors.torch import save_file
            save_file(sd, os.path.join(save_directory, "model.safetensors"), metadata={"format": "pt"})
        else:
            torch.save(sd, os.path.join(save_directory, "pytorch_model.bin"))

    def _sync_shadow(self):
        v = tuple(p._version for p in self._param_list)
        if v != self._versions:
            self.store.refresh_shadow()  # fp32 master (possibly just updated by an optimizer) -> bf16 GEMM operands
            self._versions = v

    def forward(self, input_features=None, attention_mask=None, decoder_input_ids=None, labels=None,
                encoder_outputs=None, valid_len=None, **kwargs):
        """`valid_len` (optional, HOST integers from the collator -- DataCollatorSpeechSeq2SeqWithPadding(report_valid_len=...)
        puts them into the batch, so the reference's `student_model(**batch)` / `teacher_model(**batch)` pass them on): one
        int = 1 + the last labelled position of the batch, or one per sequence.  The decoder positions behind them are dead
        (distill.trim_dead_positions) and are not computed; `.logits` keeps the reference shape [B, T, V] with zero rows there,
        `.loss` and the gradients are those of the full-length forward.  Absent: every position is computed."""
        d = self.dims
        if labels is not None:
            if labels.shape[1] > d.max_tgt:
                raise ValueError(f"Labels' sequence length {labels.shape[1]} cannot exceed the maximum allowed length "
                                 f"of {d.max_tgt} tokens.")
            if decoder_input_ids is None:
                from .distill import shift_tokens_right
                decoder_input_ids = shift_tokens_right(labels, d.pad_token_id, d.decoder_start_token_id)
        if decoder_input_ids is None:
            raise ValueError("decoder_input_ids or labels are required")
        enc_in = None
        if encoder_outputs is not None:
            enc_in = encoder_outputs[0] if not torch.is_tensor(encoder_outputs) else encoder_outputs
        elif input_features is None:
            raise ValueError("input_features or encoder_outputs are required")
        elif input_features.shape[-1] != 2 * d.max_src:
            raise ValueError(f"Whisper expects the mel input features to be of length {2 * d.max_src}, but found "
                             f"{input_features.shape[-1]}. Make sure to pad the input mel features to {2 * d.max_src}.")
        self._sync_shadow()
        if attention_mask is not None and enc_in is None and self.training and self.engine.spec is not None:
            from .spec_augment import lengths_from_attention_mask
            self._spec_lengths = lengths_from_attention_mask(attention_mask)       # (on the device: no round trip)
        if valid_len is None and labels is not None and self.skip_dead_positions and labels.shape == decoder_input_ids.shape:
            sel = _PendingLens(labels)           # (resolved inside _EngineFn.forward, behind the encoder's launches)
            if sel.lens is not None:             # the other model already fetched them for this very tensor
                sel = _RowSel.make(sel.lens, decoder_input_ids.shape[0], decoder_input_ids.shape[1], decoder_input_ids.device)
        else:
            sel = _RowSel.make(valid_len, decoder_input_ids.shape[0], decoder_input_ids.shape[1], decoder_input_ids.device)
        logits, enc = _EngineFn.apply(self, input_features, enc_in, decoder_input_ids, sel, *self._param_list)
        sel, self._last_sel = self._last_sel, None
        lowp, self._last_logits_lowp = self._last_logits_lowp, None
        state, self._last_lazy_state = self._last_lazy_state, None
        loss = None
        if labels is not None:
            # token-mean CE over labels != -100 (TF:modeling_whisper.py:1083-1087) by a forward-only pass of the fused loss
            # kernel; its gradient is produced -- together with the KD term's, if the caller adds one -- by the engine
            # node's backward (lazy_logits.lazy_backward)
            state.labels = labels
            B, T = labels.shape
            lab = state.select_rows(labels.reshape(B * T, 1)).reshape(-1).contiguous()
            loss = _CEFn.apply(logits, state, lab)
        return Seq2SeqLMOutput(loss=loss, logits=LazyLogits.wrap(logits, state), encoder_last_hidden_state=enc,
                               _logits_lowp=lowp, _model=self, _rows=sel, _lazy=state)

    @torch.no_grad()
    def teacher_topk(self, input_features=None, *, labels=None, decoder_input_ids=None, k=32, temperature=2.0,
                     encoder_outputs=None, valid_len=None):
        """Stored top-k teacher targets (topk_distill.TeacherTopK, the format of include/dwamd.h) of a batch, from the model a
        labelling job already holds: one teacher-forced pass without saved activations, then one `logits_topk` launch over its
        logits.  Given `labels`, the decoder inputs are the labels shifted right, as the trainer builds them; `valid_len` (one int
        or one per sequence, distill.trim_dead_positions) leaves the dead positions out -- they stay zero in the result and are
        never read.  A trainer uses the result as `teacher_topk=` at the same temperature."""
        from . import topk_distill
        from .distill import shift_tokens_right, trim_dead_positions
        from .engine import LiveRows
        d = self.dims
        k = topk_distill.check_k(k, d.vocab)
        if not float(temperature) > 0.0:
            raise ValueError(f"temperature > 0, got {temperature!r}")
        if decoder_input_ids is None:
            if labels is None:
                raise ValueError("decoder_input_ids or labels are required")
            decoder_input_ids = shift_tokens_right(labels, d.pad_token_id, d.decoder_start_token_id)
        if decoder_input_ids.shape[1] > d.max_tgt:
            raise ValueError(f"the sequence length {decoder_input_ids.shape[1]} exceeds the model's {d.max_tgt} positions")
        self._sync_shadow()
        if encoder_outputs is not None:
            enc, _ = self._given_encoder_output(encoder_outputs)
        elif input_features is None:
            raise ValueError("input_features or encoder_outputs are required")
        else:
            enc, _ = self.engine.encode(input_features.to(torch.float32).contiguous(), save=False)
        B, T = decoder_input_ids.shape
        ids, _, lens = trim_dead_positions(decoder_input_ids, decoder_input_ids, valid_len)
        Td = ids.shape[1]
        live = LiveRows.build(lens, Td, ids.device) if lens is not None and sum(lens) < B * Td else None
        logits, _ = self.engine.decode(ids.contiguous(), enc, save=False, live=live)
        R = B * Td if live is None else live.n
        idx, logp, rest = topk_distill.logits_topk(self.ops, logits[:R], d.vocab, temperature, k)
        idx, logp, rest = topk_distill.scatter_targets(idx, logp, rest, B, T, None if live is None else live.idx, Td)
        return topk_distill.TeacherTopK(idx, logp, rest, float(temperature), d.vocab)

    @torch.no_grad()
    def generate(self, input_features=None, generation_config=None, logits_processor=None, stopping_criteria=None,
                 prefix_allowed_tokens_fn=None, synced_gpus=False, return_timestamps=None, task=None, language=None,
                 is_multilingual=None, prompt_ids=None, prompt_condition_type=None, condition_on_prev_tokens=None,
                 temperature=None, compression_ratio_threshold=None, logprob_threshold=None, no_speech_threshold=None,
                 num_segment_frames=None, attention_mask=None, time_precision=0.02, time_precision_features=0.01,
                 return_token_timestamps=None, return_segments=False, return_dict_in_generate=None,
                 force_unique_generate_call=None, monitor_progress=None, *, use_graphs=None, cross_kv_dtype=None, seek_slots=None,
                 **kwargs):
        """`WhisperGenerationMixin.generate` (TF:generation_whisper.py:383-968) on the MI355X engine, with the argument
        list of the reference (run_distillation.py:1524-1528, run_eval.py:690-739, 806-844): greedy search over one
        30 s window per row with language / task / timestamp / prompt_ids prefixes, the suppress / begin-suppress /
        min-new-tokens / timestamp logits rules, `assistant_model` (speculative decoding), `encoder_outputs`.
        `assistant_per_row=True` (with an assistant, single window, KV caches): every row of the batch accepts its own agreeing
        draft prefix instead of the batch minimum and ends at its own EOS (decoding.assisted_greedy_decode `per_row`); without an
        assistant a ValueError, inside the seek loop or with `use_cache=False` a NotImplementedError before anything is decoded.
        The token loop is decoding.GreedyDecoder (KV cache; `use_graphs` replays the per-position launch sequence from
        HIP graphs; `use_cache=False` re-decodes the whole prefix every step and exists as a cross-check).
        `num_beams > 1` runs decoding.beam_search_decode (TF `_beam_search`; its step is two kernel entries, dw_beam_candidates and
        dw_beam_update, DW_BEAM_TORCH=1 keeps the torch step); in the seek loop it combines with the fallback thresholds, the beam
        pass being judged by its hypothesis' `sequences_scores`.  `return_timestamps=True` (without
        `force_unique_generate_call`) and inputs longer than 30 s run the reference's timestamp seek loop
        (`seek_decode`, TF:784-903) with `condition_on_prev_tokens`, the fallback thresholds (`temperature` tuple,
        `compression_ratio_threshold`, `logprob_threshold`) and the `no_speech_threshold` skip.
        Greedy decoding also takes GenerationMixin's `repetition_penalty` and `no_repeat_ngram_size`, in one window and in the
        seek loop: the selection kernel applies them (dw_greedy_select_history), so `use_graphs=True` holds with them.
        `sequence_bias` / `bad_words_ids` (SequenceBiasLogitsProcessor / NoBadWordsLogitsProcessor: hot-word boosts and forbidden
        words; at most 1024 sequences of at most 32 tokens): greedy decoding, in one window and in the seek loop, applies them in
        the same selection launch (dw_greedy_select_bias), so `use_graphs=True` holds; the seek loop's sampled fallback passes
        apply them as torch ops.  Combined with beams, an assistant, plain sampling, `use_cache=False`, `output_scores` /
        `output_logits`, `return_token_timestamps`, or `condition_on_prev_tokens=True` over several utterances they RAISE.
        Single-window decoding takes plain sampling as well (a positive `temperature`, as in the reference's
        generate_with_fallback, with `top_k` / `top_p`): decoding.GreedyDecoder `soft`.  The selection kernel samples as well
        (dw_sample_select: processors, warpers and the draw in one launch on Exponential(1) noise that torch's generator draws,
        which is what `torch.multinomial` does for one draw per row), so `use_graphs=True` holds; DW_SAMPLE_TORCH=1 keeps the
        eager torch ops.  The tokens are those of the torch ops on the same device and seed, except where the top-p boundary
        cuts through a group of equal scores (the kernel keeps the group whole, the reference's sort splits it).
        Arguments this path does not implement RAISE (nothing is silently ignored): group beam search, those three options
        combined with beams / an assistant / `use_cache=False`, plain sampling inside the seek loop, the two history options with
        `condition_on_prev_tokens=True` over several utterances, the fallback heuristics outside the seek loop, custom logits
        processors, `return_token_timestamps` combined with beams / an assistant / sampling / the fallback heuristics.
        `output_scores=True` / `output_logits=True` with `return_dict_in_generate=True` (single-window greedy search, with or
        without the KV cache, HIP graphs, prompt_ids / decoder_input_ids / encoder_outputs, the timestamp rules under
        `force_unique_generate_call`, together with `return_token_timestamps`): `.scores` / `.logits` hold one f32 [batch, vocab]
        tensor per generated step as in GenerationMixin, computed by one more teacher-forced decoder pass and csrc/score.hip
        (scoring.py; a near tie may therefore rank another token first than the token step did).  Combined with beam search,
        an assistant_model, sampling / repetition_penalty / no_repeat_ngram_size or the timestamp seek loop they RAISE; without
        `return_dict_in_generate` they change nothing (the reference drops them there too).
        `return_token_timestamps=True` (greedy; single window and the seek loop; TF:241-381): one more decoder pass over the
        finished sequences and three kernels (alignment.extract_token_timestamps) -- the result is a dict {"sequences",
        "token_timestamps"[, "segments"]} as in the reference (TF:941-968); `attention_mask` gives the valid frames per row;
        `alignment_heads=[[layer, head], ...]` may be passed like any other generation-config field.
        `cross_kv_dtype="fp8"` (None / "bf16": today's cache): the KV-cache decoder keeps the cross-attention K/V as e4m3fn codes
        with one scale per column (include/dwamd.h; README "FP8 cross-attention K/V") -- half the bytes the token step streams.
        Opt-in: it changes the numerics of the token step, so a token may differ where two logits are close.  Single-window greedy
        or sampled decoding on the KV cache, with or without graphs, with the timestamp rules under `force_unique_generate_call`
        and the repetition / bias options.  The seek loop, `num_beams > 1`, an `assistant_model`, `output_scores` /
        `output_logits` and `return_token_timestamps` RAISE NotImplementedError before the encoder runs; `use_cache=False`, any
        other value and a model width without the kernel are a ValueError.
        `seek_slots=N` (with `return_timestamps=True`, inputs of any length): the seek loop's windows as jobs of a
        decoding.SlotDecoder of N slots (seek_decode `slots`) -- an utterance's next window takes a free slot as soon as the
        previous one has ended, the token steps replay from a HIP graph, `cross_kv_dtype="fp8"` is allowed, and
        `logprob_threshold` / `no_speech_threshold` are judged on numbers the slot step keeps (dw_slot_step_scores) instead of a
        teacher-forced pass.  Greedy at temperature 0: with a positive temperature, `condition_on_prev_tokens`, beams, an
        assistant, `return_token_timestamps`, the history / bias rules, `use_cache=False`, `output_scores` / `output_logits` or
        `decoder_input_ids` it RAISES NotImplementedError before the encoder runs; without `return_timestamps` or below 1 a
        ValueError.
        Returns what the reference returns: the generated tokens only (decoder prompt and EOS stripped, right-padded
        with pad_token_id), or with `return_dict_in_generate=True` / `force_unique_generate_call=True` the full
        sequences (prompt + generated, as GenerationMixin emits them)."""
        from . import decoding
        from . import generation as G
        from . import seek
        self._sync_shadow()
        eng, d = self.engine, self.dims
        # ---- every argument resolved once; what the engine path does not run is refused here (generation.REFUSALS)
        p = G.resolve_generate(
            d, generation_config if generation_config is not None else self.generation_config, kwargs,
            input_features=input_features, return_timestamps=return_timestamps, task=task, temperature=temperature,
            unimplemented=dict(logits_processor=logits_processor, stopping_criteria=stopping_criteria,
                               prefix_allowed_tokens_fn=prefix_allowed_tokens_fn, monitor_progress=monitor_progress),
            condition_on_prev_tokens=condition_on_prev_tokens, compression_ratio_threshold=compression_ratio_threshold,
            logprob_threshold=logprob_threshold, no_speech_threshold=no_speech_threshold, attention_mask=attention_mask,
            time_precision=time_precision, return_token_timestamps=return_token_timestamps, return_segments=return_segments,
            return_dict_in_generate=return_dict_in_generate, force_unique_generate_call=force_unique_generate_call,
            use_graphs=use_graphs, cross_kv_dtype=cross_kv_dtype, seek_slots=seek_slots)
        gc, num_beams = p.gc, p.num_beams
        # ---- encoder
        encoder_outputs = kwargs.get("encoder_outputs")
        if encoder_outputs is not None:
            G.refuse(p, "encoder_outputs")
            enc, B = self._given_encoder_output(encoder_outputs)
            dev = enc.device
        else:
            if input_features is None:
                raise ValueError("input_features or encoder_outputs are required")
            frames = input_features.shape[-1]
            if frames > 2 * d.max_src and not p.return_timestamps:
                raise ValueError(
                    "You have passed more than 3000 mel input features (> 30 seconds) which automatically enables "
                    "long-form generation which requires the model to predict timestamp tokens. Please either pass "
                    "`return_timestamps=True` or make sure to pass no more than 3000 mel input features.")
            if prompt_condition_type is not None:
                if prompt_condition_type not in ("first-segment", "all-segments"):
                    raise ValueError("`prompt_condition_type` must be either 'first-segment' or 'all-segments'")
                gc.prompt_condition_type = prompt_condition_type
            if frames > 2 * d.max_src or (p.return_timestamps and not force_unique_generate_call):
                # the reference's seek loop (TF:784-903): with timestamps every window is decoded until its audio is
                # consumed, also when the input is a single 30 s window (run_pseudo_labelling.py:861-996 calls it so)
                p.seek_loop = True
                p.all_segments = getattr(gc, "prompt_condition_type", "first-segment") == "all-segments"
                G.refuse(p, "seek_loop", "all_segments", "assistant")
                return seek.generate_seek_loop(self, p, input_features, attention_mask, language, task, is_multilingual,
                                               prompt_ids, kwargs, return_segments)
            p.single_window = True
            G.refuse(p, "single_window")
            if frames != 2 * d.max_src:
                raise ValueError(f"Whisper expects the mel input features to be of length {2 * d.max_src}, but found "
                                 f"{frames}. Make sure to pad the input mel features to {2 * d.max_src}.")
            B, dev = input_features.shape[0], input_features.device
            enc, _ = eng.encode(input_features.to(torch.float32).contiguous(), save=False)
        # ---- decoder prompt (TF:1384-1608, 1853-1918)
        if p.return_timestamps and not hasattr(gc, "no_timestamps_token_id"):
            raise ValueError(G.NO_TIMESTAMPS_TOKEN)
        gc.return_timestamps = bool(p.return_timestamps)
        G.set_language_and_task(gc, language, task, is_multilingual)
        if prompt_condition_type is not None and prompt_condition_type not in ("first-segment", "all-segments"):
            raise ValueError("`prompt_condition_type` must be either 'first-segment' or 'all-segments'")
        if kwargs.get("decoder_input_ids") is not None:
            ids = kwargs["decoder_input_ids"].to(dev).long().clone()
        else:
            rows = G.retrieve_init_tokens(gc, B, lambda: self._detect_language(enc, B, gc))
            ids = torch.as_tensor(rows, dtype=torch.long, device=dev)
            if prompt_ids is not None:
                pr = torch.as_tensor(prompt_ids, dtype=torch.long, device=dev).reshape(-1)
                ids = torch.cat([pr[None, :].expand(B, -1), ids], 1)
        P = ids.shape[1]
        max_new, min_new = G.resolve_lengths(gc, P, d.max_tgt, "max_length" in kwargs)
        eos, pad = gc.eos_token_id, gc.pad_token_id
        if isinstance(eos, (list, tuple)):
            if len(eos) != 1:
                raise NotImplementedError("several eos_token_id values are not implemented on the MI355X path")
            eos = eos[0]
        if pad is None:
            pad = eos
        suppress = list(gc.suppress_tokens) if gc.suppress_tokens else None
        begin_suppress = list(gc.begin_suppress_tokens) if gc.begin_suppress_tokens else None
        assistant_model, use_graphs = p.assistant_model, bool(use_graphs)
        ts_rules = None                        # (single window with timestamps: force_unique_generate_call)
        if gc.return_timestamps:
            ts_rules = G.timestamp_rules(gc.no_timestamps_token_id, getattr(gc, "max_initial_timestamp_index", None), begin_index=P)
        if ts_rules is not None and eos is None and num_beams == 1 and (assistant_model is not None or p.use_cache):
            raise ValueError("return_timestamps=True needs eos_token_id in the generation config")
        # ---- one of four token loops
        if num_beams > 1:
            # beam search (run_eval.py:143, 693; run_distillation.py:1428-1436): TF `_beam_search` on the KV-cache decoder
            G.refuse(p, "assistant")
            if eos is None:
                raise ValueError("beam search needs eos_token_id in the generation config")
            lp = getattr(gc, "length_penalty", None)
            es = getattr(gc, "early_stopping", False)
            seqs = decoding.beam_search_decode(eng, enc, ids, max_new, num_beams, eos, pad_token_id=pad, suppress_tokens=suppress,
                                               begin_suppress_tokens=begin_suppress, min_new_tokens=min_new,
                                               length_penalty=1.0 if lp is None else float(lp),
                                               early_stopping=False if es is None else es, timestamp_rules=ts_rules)
        elif assistant_model is not None:
            begin_suppress = None          # TF:719-721: the model must be able to return EOS right away
            seqs = self._assisted_decode(p, enc, ids, input_features, max_new, min_new, eos, pad, suppress, ts_rules)
        elif p.use_cache:
            seqs = self._cached_decode(p, enc, ids, max_new, min_new, eos, pad, suppress, begin_suppress, ts_rules, use_graphs)
        else:
            if gc.return_timestamps:
                raise ValueError("return_timestamps=True runs on the KV-cache decoder (use_cache=True)")
            seqs = decoding.greedy_no_cache(eng, d.vocab, enc, ids, max_new, min_new, eos, pad, suppress, begin_suppress)
        seqs = G.trim_finished(seqs, P, eos, pad)
        return self._generate_result(p, seqs, enc, P, min_new, eos, pad, suppress, begin_suppress, force_unique_generate_call)

    def _given_encoder_output(self, enc):
        """`generate(encoder_outputs=)`: a tensor, a BaseModelOutput or a tuple -> (rows in the dtype `encode` returns, B)."""
        d = self.dims
        if not torch.is_tensor(enc):
            enc = enc.last_hidden_state if hasattr(enc, "last_hidden_state") else enc[0]
        B = enc.shape[0] if enc.dim() == 3 else enc.shape[0] // d.max_src
        if enc.numel() != B * d.max_src * d.d_model:
            raise ValueError(f"encoder_outputs must cover {d.max_src} positions of width {d.d_model} per row")
        return enc.reshape(-1, d.d_model).to(self.engine.lowp).contiguous(), B      # (GEMM operand)

    def _cached_decode(self, p, enc, ids, max_new, min_new, eos, pad, suppress, begin_suppress, ts_rules, use_graphs):
        """Greedy or sampled decoding on the model's one live decoding.GreedyDecoder, rebuilt when its key changes."""
        from .decoding import GreedyDecoder
        B, total = ids.shape[0], ids.shape[1] + max_new
        key = (B, total, eos, pad, use_graphs, tuple(suppress or ()), tuple(begin_suppress or ()),
               None if ts_rules is None else tuple(sorted(ts_rules.items())),
               None if p.soft is None else tuple(sorted((k, v) for k, v in p.soft.items())), p.cross_kv_dtype)
        dec = self._decoders.get(key)
        if dec is None:
            dec = GreedyDecoder(self.engine, B, total, eos_token_id=eos, suppress_tokens=suppress,
                                begin_suppress_tokens=begin_suppress, use_graphs=use_graphs, check_every=16 if use_graphs else 1,
                                timestamp_rules=ts_rules, pad_token_id=pad, soft=p.soft, cross_kv_dtype=p.cross_kv_dtype)
            self._decoders = {key: dec}        # one live decoder (its graphs pin the K/V cache buffers)
        return dec.run(enc, ids, max_new, min_new)

    def _assisted_decode(self, p, enc, ids, input_features, max_new, min_new, eos, pad, suppress, ts_rules):
        """Speculative decoding (run_eval.py:578-599, 706-707): the assistant drafts, this model verifies.  An assistant with
        this model's encoder dimensions re-uses the encoder output (the distilled student keeps a frozen copy of the teacher's
        encoder); otherwise it encodes the features itself."""
        from .decoding import assisted_greedy_decode
        am, d, gc = p.assistant_model, self.dims, p.gc
        am._sync_shadow()
        if _assistant_shares_encoder(am, d) or (input_features is None and am.dims.d_model == d.d_model):
            enc_a = enc.to(am.engine.lowp)
        else:
            if input_features is None:
                raise ValueError("the assistant needs input_features (its encoder differs from this model's)")
            enc_a, _ = am.engine.encode(input_features.to(torch.float32).contiguous(), save=False)
        k = getattr(gc, "num_assistant_tokens", None) or \
            getattr(getattr(am, "generation_config", None), "num_assistant_tokens", None) or 5
        seqs, self.last_drafted, self.last_accepted = assisted_greedy_decode(
            self.engine, am.engine, enc, enc_a, ids, max_new, int(k), eos, suppress_tokens=suppress,
            min_new_tokens=min_new, pad_token_id=pad, timestamp_rules=ts_rules, per_row=p.per_row)
        return seqs

    def _generate_result(self, p, seqs, enc, P, min_new, eos, pad, suppress, begin_suppress, unique_call):
        """What `generate` returns for a single window, shaped as the reference shapes it (TF:913-968)."""
        from . import generation as G
        gc, token_ts = p.gc, p.token_ts
        step_scores = step_logits = None
        if p.want_scores or p.want_logits:
            # one teacher-forced pass over the finished sequences + csrc/score.hip (scoring.py says why a second pass)
            from .scoring import score_sequences
            sc_rules = None
            if gc.return_timestamps:
                sc_rules = G.timestamp_rules(gc.no_timestamps_token_id, getattr(gc, "max_initial_timestamp_index", None))
            step_scores, step_logits = score_sequences(
                self, seqs, enc, P, dict(suppress_tokens=suppress, begin_suppress_tokens=begin_suppress, min_new_tokens=min_new,
                                         eos_token_id=eos, timestamp_rules=sc_rules), p.want_scores, p.want_logits)
        if token_ts is not None:
            # TF:1146-1157: one alignment pass over the finished sequences
            from .alignment import extract_token_timestamps
            ts = extract_token_timestamps(self, seqs, enc, token_ts["alignment_heads"], token_ts["num_frames"], P,
                                          token_ts["time_precision"])
            if p.as_dict:
                return G.GenerateOutput(seqs, scores=step_scores, token_timestamps=ts, logits=step_logits)
            if unique_call:
                return {"sequences": seqs, "token_timestamps": ts}
            plain, plain_ts = G.strip_and_pad(seqs, P, eos, pad, token_timestamps=ts)
            return {"sequences": plain, "token_timestamps": plain_ts}
        if p.as_dict:
            return G.GenerateOutput(seqs, scores=step_scores, logits=step_logits)
        return seqs if unique_call else G.strip_and_pad(seqs, P, eos, pad)

    def compute_transition_scores(self, sequences, scores, beam_indices=None, normalize_logits=False):
        """`GenerationMixin.compute_transition_scores`: f32 [batch, steps], the score of every generated token of `sequences` in
        `scores` (what `generate(output_scores=True, return_dict_in_generate=True)` returned as `.scores` or `.logits`), its
        log-probability with `normalize_logits=True`.  For this package's tuples these are the values csrc/score.hip computed
        next to the scores; foreign tensors go through the reference's gather.  `beam_indices` raises (no scores under beams)."""
        from .scoring import compute_transition_scores
        return compute_transition_scores(sequences, scores, beam_indices, normalize_logits)

    def seek_decode(self, input_features, max_frames, init_tokens, lengths, eos, pad, no_timestamps_token_id,
                    max_initial_timestamp_index=None, suppress_tokens=None, begin_suppress_tokens=None,
                    detect_language=None, temperatures=(0.0,), compression_ratio_threshold=None, logprob_threshold=None,
                    no_speech_threshold=None, condition_on_prev_tokens=False, prev_sot_token_id=None, prompt_ids=None,
                    prompt_all_segments=False, num_beams=1, length_penalty=1.0, early_stopping=False, assistant=None,
                    num_assistant_tokens=5, token_timestamps=None, repetition_penalty=None, no_repeat_ngram_size=0,
                    sequence_bias=None, slots=None, check_every=8, cross_kv_dtype=None, use_graphs=None):
        """The seek loop itself (TF:generation_whisper.py:784-903): input_features [B, n_mels, frames], max_frames[b] =
        valid mel frames of utterance b.  init_tokens: the decoder prompt rows (list of B lists) or a callable(detect)
        building them (detect() = language ids from the first window); lengths(P) -> (max_new_tokens, min_new_tokens)
        for a decoder prompt of P tokens.  Every pass encodes the next <= 30 s window of each unfinished utterance,
        decodes it with the timestamp rules and advances that utterance by what `retrieve_segment` says it consumed.
          * condition_on_prev_tokens (TF:1853-1918): the tokens of the utterance's earlier segments (last 223, behind
            <|startofprev|>) precede the prompt.  The reference left-pads a batch and masks the pads; rows are
            independent, so here rows are decoded in groups of equal prompt length (no pads, same positions);
          * fallback (TF:970-1116, 1243-1287): a window whose zlib compression ratio of the token bytes exceeds
            `compression_ratio_threshold` or whose average log-probability is below `logprob_threshold` is decoded
            again at the next temperature (sampling; the random stream is this process's, not the reference's; each step is one
            noise draw and one dw_sample_select launch where the ops have it);
            `no_speech_threshold`: P(<|nospeech|>) after <|startoftranscript|> above it together with a low average
            log-probability skips the window.  The scores are recomputed by one teacher-forced decoder pass.
          * prompt_ids (`processor.get_prompt_ids`, run_eval.py:709-710; prompt_condition_type "first-segment"): without
            conditioning on previous tokens the prompt precedes the decoder prompt of EVERY window (TF:1909-1911); with
            it the prompt is the utterance's segment zero (TF:1119-1123), so it conditions the following windows like
            any earlier text until the 223-token cut-off pushes it out, and is dropped from the result (TF:906-910);
            prompt_all_segments (prompt_condition_type "all-segments", needs condition_on_prev_tokens): the prompt takes
            the place of <|startofprev|> in front of the previous tokens of every window (TF:1887-1888);
          * num_beams > 1 (run_eval.py:693 / run_pseudo_labelling.py `--generation_num_beams`): the temperature-0 pass of a
            window is a beam search (decoding.beam_search_decode with the timestamp rules); sampled fallback passes use
            one beam like the reference (TF:1004-1005).  With `logprob_threshold` the beam pass is judged by its hypothesis'
            `sequences_scores` (the length-penalised sum of log-probabilities) instead of the average token log-probability,
            without a rescoring pass; the no-speech probability comes from the beam search's own prompt prefill
            (`beam_no_speech` below says which row the reference reads); sampled passes are scored as without beams.
            A DELIBERATE DEVIATION from the installed reference: `_need_fallback` (TF:1261-1273) states this rule -- `if
            hasattr(seek_outputs[0], "sequences_scores")` -- but its per-window outputs are plain dicts, the test is false, and
            `transformers` 5.15 instead averages, by `_retrieve_avg_logprobs`, the processed scores of EXPANDED row `index` of
            the B * num_beams beam rows (the beam in slot `index % num_beams` of utterance `index // num_beams` at each step)
            at the window's own tokens: a number that belongs to no hypothesis.  This package follows the stated rule, not that
            number, so for a `logprob_threshold` between a window's `sequences_scores` and that average its fallback / skip
            decision differs from the installed reference's.  tests/golden/beam_thresholds.json is made with the stated
            branch reachable and records one such threshold per multilingual seed together with what the untouched reference
            returns there (`installed_differs`); tests/test_beam_step.py pins both;
          * assistant = (engine, encode) of a draft model (run_eval.py:578-599, 706-707 with long-form inputs): the
            temperature-0 pass of a window is decoding.assisted_greedy_decode with the timestamp rules; encode(features)
            gives the assistant's encoder output of a window batch, or None when it shares this model's.
          * token_timestamps = dict(alignment_heads, num_frames, time_precision) (greedy passes only): every window's finished
            batch goes through alignment.extract_token_timestamps with `num_frames - seek` of its rows (TF:1146-1157); a segment
            then carries "token_timestamps" (its tokens' times plus the window's offset, TF:2034-2036, 2068-2070) and, as in the
            reference, "result" = {"token_timestamps": the window's row} with "idxs" = the segment's slice of it.
          * repetition_penalty / no_repeat_ngram_size (the reference hands its generation config to GenerationMixin.generate for
            every window, TF `generate_with_fallback`): the greedy pass of a window runs them inside the selection kernel
            (decoding.GreedyDecoder `soft`), over the window's decoder prompt and tokens -- previous-text prompt included;
            sampled fallback passes apply them in the sampling kernel (or through `processed` on the torch path) and the
            threshold scores see them through `processed`.  Not with beams or an assistant,
            and not with condition_on_prev_tokens over several utterances (see the message below).
          * sequence_bias (a decoding.SequenceBiasTable: `generate(sequence_bias=, bad_words_ids=)`): under the same conditions;
            the greedy pass of a window applies the table inside the selection kernel (dw_greedy_select_bias), the sampled
            fallback passes and the threshold scores apply it as torch ops through `processed` (the sampling kernel takes no
            table).  Not with token timestamps.
          * slots=N (None: the lockstep loop above, pass by pass): the same windows as jobs of a decoding.SlotDecoder of N slots.
            Every (utterance, window) is decoded by the slot step with the timestamp rules at the slot's own position; when a
            window ends, `retrieve_segment` tells the utterance's next window, which joins the windows still to encode
            (continuations before utterances not yet started).  The encoder runs when no encoded window is waiting, over up to
            N windows in one call, so at most 2 N encoded windows exist (N in slots, N waiting).  A short tail window therefore
            waits for no longer row of its pass, the token steps replay from a HIP graph (`use_graphs`), and
            `cross_kv_dtype="fp8"` keeps the slots' cross-attention K/V as FP8 codes.  With the thresholds the slot step itself
            keeps each window's log-probability sum and no-speech probability (dw_slot_step_scores): no teacher-forced pass.
            Greedy, temperature 0 only: a positive temperature, condition_on_prev_tokens, beams, an assistant, token timestamps,
            the history / bias rules raise NotImplementedError before the encoder runs, as do `init_tokens` rows of different
            lengths.  `last_seek_stats` holds the token steps, the encoder calls' batch sizes and the most encoded windows held;
            `last_window_scores` (either loop, with a threshold) the numbers every window was judged by.
        -> per utterance the list of segments {"start", "end", "tokens"}."""
        from . import seek
        return seek.seek_decode(self, dict(
            input_features=input_features, max_frames=max_frames, init_tokens=init_tokens, lengths=lengths, eos=eos, pad=pad,
            no_timestamps_token_id=no_timestamps_token_id, max_initial_timestamp_index=max_initial_timestamp_index,
            suppress_tokens=suppress_tokens, begin_suppress_tokens=begin_suppress_tokens, detect_language=detect_language,
            temperatures=temperatures, compression_ratio_threshold=compression_ratio_threshold,
            logprob_threshold=logprob_threshold, no_speech_threshold=no_speech_threshold,
            condition_on_prev_tokens=condition_on_prev_tokens, prev_sot_token_id=prev_sot_token_id, prompt_ids=prompt_ids,
            prompt_all_segments=prompt_all_segments, num_beams=num_beams, length_penalty=length_penalty,
            early_stopping=early_stopping, assistant=assistant, num_assistant_tokens=num_assistant_tokens,
            token_timestamps=token_timestamps, repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size,
            sequence_bias=sequence_bias, slots=slots, check_every=check_every, cross_kv_dtype=cross_kv_dtype,
            use_graphs=use_graphs))

    # -- helpers of generate ----------------------------------------------------------------------------------------
    def _detect_language(self, enc, B, gc):
        """TF:1610-1674 `detect_language`: one decoder step on <|startoftranscript|>, argmax over the language ids."""
        d = self.dims
        ids = torch.full((B, 1), gc.decoder_start_token_id, dtype=torch.long, device=enc.device)
        logits, _ = self.engine.decode(ids, enc, save=False)
        sc = logits[:B, : d.vocab].float()
        lang_ids = torch.as_tensor(sorted(gc.lang_to_id.values()), dtype=torch.long, device=enc.device)
        mask = torch.full((d.vocab,), float("-inf"), device=enc.device)
        mask[lang_ids] = 0.0
        return (sc + mask).argmax(-1).tolist()


@dataclass
class CausalLMOutput:
    logits: torch.Tensor = None

    def __getitem__(self, i):
        return (self.logits,)[i]


class _DecoderWrapper(nn.Module):                  # TF:modeling_whisper.py `WhisperDecoderWrapper`: the keys are model.decoder.*
    def __init__(self, d):
        super().__init__()
        self.decoder = _Decoder(d)


class WhisperForCausalLM(nn.Module):
    """The decoder-only drop-in of `transformers.WhisperForCausalLM` (TF:modeling_whisper.py): the class the reference loads the
    distilled student with when it drafts for the teacher (run_eval.py:578-599, README "speculative decoding").  It holds the
    decoder and the tied LM head and NO encoder parameter -- the flat store is built over the `model.decoder.*` entries
    (`ParamStore(decoder_only=True)`), so no copy of an encoder exists on the device.  Inference only: `forward(input_ids,
    encoder_outputs=)` -> `.logits`; as `generate(assistant_model=)` of a `WhisperForConditionalGeneration` it always drafts on
    that model's encoder output and needs the same d_model.  `generate` on the class itself is not implemented."""

    decoder_only = True

    def __init__(self, config, ops=None, device="cuda:0", state_dict=None, seed=0, dtype=torch.float32):
        super().__init__()
        check_regularisers(config)
        self.config = config
        self.dims = WhisperDims.from_any(config)
        self.ops = ops if ops is not None else _default_ops(device)
        if dtype not in (torch.float32, torch.bfloat16, None):
            raise ValueError(f"dtype {dtype}: the MI355X path computes in bf16 with fp32 or bf16 parameters")
        self.dtype_mode = torch.float32 if dtype is None else dtype
        pure_bf16 = self.dtype_mode == torch.bfloat16
        if state_dict is None:
            import dataclasses
            state_dict = random_state_dict(dataclasses.replace(self.dims, enc_layers=0), seed, device=self.ops.device)
        sd = {k: v for k, v in state_dict.items() if k.startswith("model.decoder.")}      # a full checkpoint's encoder is ignored
        if "model.decoder.embed_tokens.weight" not in sd and "proj_out.weight" in state_dict:
            sd["model.decoder.embed_tokens.weight"] = state_dict["proj_out.weight"]
        self.store = ParamStore(self.ops, self.dims, sd, trainable=False, round_bf16=pure_bf16, decoder_only=True)
        self.engine = WhisperEngine(self.ops, self.store, self.ops.lowp if pure_bf16 else torch.float32)
        self.model = _DecoderWrapper(self.dims)
        self.proj_out = nn.Linear(self.dims.d_model, self.dims.vocab, bias=False, device="meta")
        for name in self.store.real_names():
            mod_path, pname = name.rsplit(".", 1)
            setattr(self.get_submodule(mod_path), pname, nn.Parameter(self.store.p[name], requires_grad=False))
        self.proj_out.weight = self.model.decoder.embed_tokens.weight  # tied (TF:modeling_whisper.py `WhisperForCausalLM`)
        self._param_list = [self.get_parameter(n) for n in self.store.real_names()]
        self._versions = None
        from .generation import GenerationConfig
        self.generation_config = GenerationConfig.from_model_config(config)

    def state_dict(self, *args, destination=None, prefix="", keep_vars=False):
        """Independent tensors under the reference class's keys, the tied `proj_out.weight` one tensor with
        `model.decoder.embed_tokens.weight` (see WhisperForConditionalGeneration.state_dict)."""
        sd = nn.Module.state_dict(self, *args, destination=destination, prefix=prefix, keep_vars=keep_vars)
        if keep_vars:
            return sd
        for k in [k for k in sd if k.startswith(prefix)]:
            sd[k] = sd[k].clone()
        sd[prefix + "proj_out.weight"] = sd[prefix + "model.decoder.embed_tokens.weight"]
        return sd

    _sync_shadow = WhisperForConditionalGeneration._sync_shadow
    save_pretrained = WhisperForConditionalGeneration.save_pretrained

    def get_decoder(self):
        return self.model.decoder

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, *model_args, config=None, torch_dtype=None, dtype=None, subfolder="",
                        variant=None, use_safetensors=None, ops=None, device="cuda:0", **kwargs):
        """Load a LOCAL checkpoint directory: a decoder-only one (`model.decoder.*`, `proj_out.weight`) or a full Whisper
        checkpoint, of which the decoder tensors are taken and `model.encoder.*` is ignored (as `transformers` loads
        `distil-whisper/*` checkpoints into this class)."""
        import os
        path = os.path.join(str(pretrained_model_name_or_path), subfolder) if subfolder else str(pretrained_model_name_or_path)
        if not os.path.isdir(path):
            raise OSError(f"{path} is not a local checkpoint directory (no hub access in this environment)")
        if config is None:
            config = WhisperConfig.from_pretrained(path)
        dt = dtype if dtype is not None else torch_dtype
        if isinstance(dt, str):
            dt = {"float32": torch.float32, "bfloat16": torch.bfloat16, "auto": None}.get(dt, dt)
        st_path = os.path.join(path, "model.safetensors" if not variant else f"model.{variant}.safetensors")
        bin_path = os.path.join(path, "pytorch_model.bin")
        if os.path.exists(st_path) and use_safetensors is not False:
            from safetensors import safe_open
            with safe_open(st_path, framework="pt") as f:                  # (the encoder tensors of a full checkpoint are not read)
                sd = {k: f.get_tensor(k) for k in f.keys() if not k.startswith("model.encoder.")}
        elif os.path.exists(bin_path):
            sd = torch.load(bin_path, map_location="cpu", weights_only=True)
        else:
            raise OSError(f"no model.safetensors / pytorch_model.bin under {path}")
        return cls(config, ops=ops, device=device, state_dict=sd, dtype=dt)

    @torch.no_grad()
    def forward(self, input_ids=None, attention_mask=None, encoder_outputs=None, **kwargs):
        """Logits [B, T, V] of the teacher-forced decoder pass over `input_ids` against `encoder_outputs` (a tensor [B, Lk, D],
        a tuple or an output object whose first entry is one).  Inference only: no `labels`, nothing is kept for a backward."""
        d = self.dims
        if kwargs.get("labels") is not None:
            raise NotImplementedError("WhisperForCausalLM is inference-only on the MI355X path (no labels / loss)")
        if input_ids is None or encoder_outputs is None:
            raise ValueError("input_ids and encoder_outputs are required (this class has no encoder)")
        enc = encoder_outputs
        if not torch.is_tensor(enc):
            enc = enc.last_hidden_state if hasattr(enc, "last_hidden_state") else enc[0]
        B, T = input_ids.shape
        if enc.numel() != B * d.max_src * d.d_model:
            raise ValueError(f"encoder_outputs must cover {d.max_src} positions of width {d.d_model} per row")
        self._sync_shadow()
        enc = enc.reshape(-1, d.d_model).to(self.engine.lowp).contiguous()
        logits, _ = self.engine.decode(input_ids.contiguous(), enc, save=False)
        return CausalLMOutput(logits=logits[: B * T, : d.vocab].float().view(B, T, d.vocab))

    def generate(self, *args, **kwargs):
        raise NotImplementedError("WhisperForCausalLM drafts for a WhisperForConditionalGeneration (`generate(assistant_model=)`); "
                                  "`generate` on the decoder-only class itself is not implemented on the MI355X path")
