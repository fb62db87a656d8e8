"""SpecAugment of the training forward (`apply_spec_augment`, `mask_time_*`, `mask_feature_*` of `transformers.WhisperConfig`;
TF:modeling_whisper.py `_compute_mask_indices`, `WhisperModel._mask_input_features`).

The span counts, the dummy index of a zero-span row and the application are the reference's; the reference draws with numpy's
global generator on the host, this path draws with the counter-based generator of the dropout kernels (Philox4x32-10 keyed by
seed, step, site, index -- include/dwamd.h dw_spec_augment states the scheme), so that the HIP kernel (csrc/spec_augment.hip,
`ops.spec_augment`) draws on the device from the device-resident step counter.  This module holds the parameter handling and
the torch statement of the same draws, which ops objects without the kernel (oracle.ref_ops, CPU runs) use.
"""
import torch

SITE_TIME, SITE_FEATURE = 512, 513          # above every dropout site (engine.drop_site < 512)
PARAM_DEFAULTS = dict(mask_time_prob=0.05, mask_time_length=10, mask_time_min_masks=2,
                      mask_feature_prob=0.0, mask_feature_length=10, mask_feature_min_masks=0)
MAX_ROWS = 65534                            # row b draws at counter words ((b + 1) << 16) | ...

_M0, _M1 = 0xD2511F53, 0xCD9E8D57
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_U32 = 0xFFFFFFFF


def params_from_config(config):
    """The six mask parameters of a config whose `apply_spec_augment` is true, else None."""
    if not getattr(config, "apply_spec_augment", False):
        return None
    return normalise({k: getattr(config, k, v) for k, v in PARAM_DEFAULTS.items()})


def normalise(params):
    """A dict of the six mask parameters (missing ones: the reference's defaults) with checked types."""
    unknown = set(params) - set(PARAM_DEFAULTS)
    if unknown:
        raise ValueError(f"spec_augment: unknown parameter(s) {sorted(unknown)}; expected {sorted(PARAM_DEFAULTS)}")
    p = dict(PARAM_DEFAULTS)
    p.update(params)
    out = {}
    for k, v in p.items():
        out[k] = float(v) if k.endswith("_prob") else int(v)
    return out


def active(params):
    return params is not None and (params["mask_time_prob"] > 0 or params["mask_feature_prob"] > 0)


def check_axis(mask_length, sequence_length):
    """The two argument errors of the reference's `_compute_mask_indices`, with its messages."""
    if mask_length < 1:
        raise ValueError("`mask_length` has to be bigger than 0.")
    if mask_length > sequence_length:
        raise ValueError(f"`mask_length` has to be smaller than `sequence_length`, but got `mask_length`: {mask_length}"
                         f" and `sequence_length`: {sequence_length}`")


def validate(params, n_mels, T):
    """As the reference: an axis is checked when it is masked (`mask_*_prob > 0`), time first."""
    if params["mask_time_prob"] > 0:
        check_axis(params["mask_time_length"], T)
    if params["mask_feature_prob"] > 0:
        check_axis(params["mask_feature_length"], n_mels)


def philox4x32_10(index, site, step, seed):
    """index: int64 tensor of counter words 0 -> int64 [..., 4], the four 32-bit output words of Philox4x32-10 with
    counter = (index, site, step_lo, step_hi) and key = seed.  (int64 products wrap modulo 2^64: the bits are those of the
    unsigned product.)"""
    step, seed = int(step) & (2**64 - 1), int(seed) & (2**64 - 1)
    c0 = index.to(torch.int64) & _U32
    c1 = torch.full_like(c0, int(site) & _U32)
    c2 = torch.full_like(c0, step & _U32)
    c3 = torch.full_like(c0, step >> 32)
    k0, k1 = seed & _U32, seed >> 32
    for _ in range(10):
        p0, p1 = c0 * _M0, c2 * _M1
        c0, c1, c2, c3 = ((p1 >> 32) & _U32) ^ c1 ^ k0, p1 & _U32, ((p0 >> 32) & _U32) ^ c3 ^ k1, p0 & _U32
        k0, k1 = (k0 + _W0) & _U32, (k1 + _W1) & _U32
    return torch.stack([c0, c1, c2, c3], -1)


def span_count(length, axis_len, prob, mask_length, min_masks, epsilon):
    """`compute_num_masked_span` of the reference (Python floats are doubles; this order of operations)."""
    n = int(prob * length / mask_length + epsilon)
    n = max(n, min_masks)
    if n * mask_length > axis_len:
        n = axis_len // mask_length
    if length - (mask_length - 1) < n:
        n = max(length - (mask_length - 1), 0)
    return n


def row_starts(seed, step, site, b, n, M):
    """n distinct starts out of [0, M) for row b in draw order: Floyd's subset algorithm over the row's Philox words."""
    if n == 0:
        return []
    w = torch.arange(n, dtype=torch.int64)
    words = philox4x32_10(((b + 1) << 16) | (w >> 2), site, step, seed).gather(1, (w & 3)[:, None])[:, 0]
    j = M - n + w
    t = ((words * (j + 1)) >> 32).tolist()
    chosen, out = set(), []
    for jj, tt in zip(j.tolist(), t):
        s = jj if tt in chosen else tt
        chosen.add(s)
        out.append(s)
    return out


def axis_mask(seed, step, site, B, axis_len, lengths, prob, mask_length, min_masks):
    """bool [B, axis_len] (True = zeroed) of one axis; lengths: B host ints or None (every row is axis_len long)."""
    check_axis(mask_length, axis_len)
    if B > MAX_ROWS:
        raise ValueError(f"spec_augment: at most {MAX_ROWS} rows")
    mask = torch.zeros(B, axis_len, dtype=torch.bool)
    epsilon = float(int(philox4x32_10(torch.zeros(1, dtype=torch.int64), site, step, seed)[0, 0])) * 2.0**-32
    if span_count(axis_len, axis_len, prob, mask_length, min_masks, epsilon) == 0:
        return mask
    for b in range(B):
        length = axis_len if lengths is None else max(0, min(axis_len, int(lengths[b])))
        n = span_count(length, axis_len, prob, mask_length, min_masks, epsilon)
        if n == 0:
            mask[b, axis_len - 1] = True            # the reference's dummy index
            continue
        for s in row_starts(seed, step, site, b, n, length - (mask_length - 1)):
            mask[b, s:s + mask_length] = True
    return mask


def masks(seed, step, B, n_mels, T, lengths, params):
    """(time mask bool [B, T] or None, feature mask bool [B, n_mels] or None) of one forward, on the host."""
    validate(params, n_mels, T)
    tm = fm = None
    if params["mask_time_prob"] > 0:
        tm = axis_mask(seed, step, SITE_TIME, B, T, lengths, params["mask_time_prob"], params["mask_time_length"],
                       params["mask_time_min_masks"])
    if params["mask_feature_prob"] > 0:
        fm = axis_mask(seed, step, SITE_FEATURE, B, n_mels, None, params["mask_feature_prob"], params["mask_feature_length"],
                       params["mask_feature_min_masks"])
    return tm, fm


def spec_augment_torch(x, seed, state, params, lengths=None, out=None, want_masks=False):
    """The torch statement behind the interface of `HipOps.spec_augment` (reads the step counter and the lengths on the host)."""
    B, n_mels, T = x.shape
    lens = None if lengths is None else [int(v) for v in lengths.tolist()]
    tm, fm = masks(seed, int(state.item()), B, n_mels, T, lens, params)
    if out is None:
        out = x
    elif out is not x:
        out.copy_(x)
    if tm is not None:
        out.masked_fill_(tm.to(x.device)[:, None, :], 0.0)
    if fm is not None:
        out.masked_fill_(fm.to(x.device)[:, :, None], 0.0)
    if not want_masks:
        return out, None, None
    tm = torch.zeros(B, T, dtype=torch.bool) if tm is None else tm
    fm = torch.zeros(B, n_mels, dtype=torch.bool) if fm is None else fm
    return out, tm.to(torch.uint8).to(x.device), fm.to(torch.uint8).to(x.device)


def lengths_from_attention_mask(attention_mask):
    """Valid frames per row as int32 on the mask's device (no host round trip)."""
    return attention_mask.sum(-1).to(torch.int32).contiguous()
