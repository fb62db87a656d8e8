"""FP8 cross-attention K/V as torch statements: quantise, dequantise and attention over `s * float(code)` in fp32.

The format is stated once, in include/dwamd.h ("FP8 cross-attention K/V"): OCP e4m3fn codes, one fp32 scale per (sequence, layer,
tensor, column) from the column's largest magnitude over the sequence's rows.  The kernels are csrc/cross_kv8.hip
(`dw_cross_kv_quant`, `dw_decode_attn_proj_kv8`); this module is what ops without them run (oracle.ref_ops, the CPU) and what the
tests hold the kernels against, next to the numpy statement tests/kv_quant_restatement.py.
"""
import torch

E4M3_MAX = 448.0
KERNEL_WIDTHS = (384, 512, 768, 1024, 1280)      # d_model with an instantiation of the token-step kernel


def normalize_dtype(cross_kv_dtype):
    """None / "bf16" -> None (the cache as it always was), "fp8" -> "fp8"; anything else is a ValueError."""
    if cross_kv_dtype is None or cross_kv_dtype == "bf16":
        return None
    if cross_kv_dtype == "fp8":
        return "fp8"
    raise ValueError(f'cross_kv_dtype must be None, "bf16" or "fp8", got {cross_kv_dtype!r}')


def check_width(d_model):
    if int(d_model) not in KERNEL_WIDTHS:
        raise ValueError(f'cross_kv_dtype="fp8" needs a model width with the token-step kernel {KERNEL_WIDTHS}, got d_model = {d_model}')


def quantize(x):
    """x [n_seq, rows, C] (bf16 values in any float dtype) -> codes uint8 [n_seq, rows, C], scales f32 [n_seq, C]."""
    x = x.to(torch.float32)
    amax = x.abs().amax(1)
    zero = amax < 2.0 ** -100                                      # (dwamd.h: such a column counts as zero; 448 / amax stays finite)
    top = torch.full_like(amax, E4M3_MAX)
    one = torch.ones_like(amax)
    inv = torch.where(zero, one, top / amax)
    s = torch.where(zero, one, amax / top)
    y = (x * inv[:, None, :]).clamp(-E4M3_MAX, E4M3_MAX)          # (torch's conversion turns what exceeds 448 into NaN: saturate first)
    codes = y.to(torch.float8_e4m3fn).view(torch.uint8)
    return codes, s


def decode(codes):
    """float(code) in fp32 (exact)."""
    return codes.view(torch.float8_e4m3fn).to(torch.float32)


def dequantize(codes, scales):
    """s * float(code): codes [n_seq, rows, C], scales [n_seq, C] -> f32 [n_seq, rows, C]."""
    return scales[:, None, :] * decode(codes)


def head_major(codes, H):
    """[n_seq, rows, 64 H] -> the cache layout [n_seq, H, rows, 64]."""
    n, r, _ = codes.shape
    return codes.view(n, r, H, 64).permute(0, 2, 1, 3).contiguous()


def quantize_into(kv, k8, v8, scales, seq0, n_seq, src_len, H):
    """What `dw_cross_kv_quant` does: kv [>= n_seq * src_len, >= 128 H] bf16 K | V rows -> the codes and scales of sequences
    [seq0, seq0 + n_seq) in the layer's buffers k8, v8 uint8 [B, H, src_len, 64], scales f32 [B, 2, 64 H]."""
    D = 64 * H
    x = kv[:n_seq * src_len, :2 * D].reshape(n_seq, src_len, 2 * D)
    codes, s = quantize(x)
    k8[seq0:seq0 + n_seq].copy_(head_major(codes[..., :D], H))
    v8[seq0:seq0 + n_seq].copy_(head_major(codes[..., D:], H))
    scales[seq0:seq0 + n_seq].copy_(s.view(n_seq, 2, D))


def attention(q, k8, v8, scales, scale, out_dtype=torch.bfloat16):
    """Cross-attention of q [B * n, 64 H] over an FP8 cache (k8, v8 uint8 [B, H, rows, 64], scales f32 [B, 2, 64 H]) -> [B * n, 64 H]
    in `out_dtype`: scores over sK * float(code) in fp32 (float64 for a float64 q), softmax, P rounded to `out_dtype` in front
    of the product with sV * float(code) -- oracle.ref_ops.attn_fwd's statement with the dequantised values in place of bf16 K/V."""
    B, H, _, _ = k8.shape
    D = 64 * H
    n = q.shape[0] // B
    ct = torch.float64 if q.dtype == torch.float64 else torch.float32
    sK = scales[:, 0].view(B, H, 1, 64).to(ct)
    sV = scales[:, 1].view(B, H, 1, 64).to(ct)
    kh, vh = sK * decode(k8).to(ct), sV * decode(v8).to(ct)
    qh = q.to(ct).view(B, n, H, 64).permute(0, 2, 1, 3)
    s = (qh @ kh.transpose(-1, -2)) * scale
    p = torch.exp(s - torch.logsumexp(s, -1)[..., None])
    o = p.to(out_dtype).to(ct) @ vh
    return o.permute(0, 2, 1, 3).reshape(B * n, D).to(out_dtype)
