"""TEST INFRASTRUCTURE -- the FP8 cross-attention K/V format of include/dwamd.h ("FP8 cross-attention K/V") in numpy, written from
the rule and independent of distil_whisper_amd/kv_quant.py (torch) and csrc/cross_kv8.hip (the kernels): the 256 values of OCP
e4m3fn written out, the quantiser in fp32 arithmetic with the rounding done by search in that table, and single-query attention
over the codes in float64.  tests/test_cross_kv_fp8.py holds the torch statement against it bit for bit, tests/
test_cross_kv_fp8_gpu.py the kernels."""
import numpy as np

# value of code c: sign c >> 7, exponent (c >> 3) & 15 (bias 7), mantissa c & 7; exponent 0: mantissa * 2^-9; 0x7f / 0xff: NaN
E4M3FN = np.array([
    0.0, 0.001953125, 0.00390625, 0.005859375, 0.0078125, 0.009765625, 0.01171875, 0.013671875,
    0.015625, 0.017578125, 0.01953125, 0.021484375, 0.0234375, 0.025390625, 0.02734375, 0.029296875,
    0.03125, 0.03515625, 0.0390625, 0.04296875, 0.046875, 0.05078125, 0.0546875, 0.05859375,
    0.0625, 0.0703125, 0.078125, 0.0859375, 0.09375, 0.1015625, 0.109375, 0.1171875,
    0.125, 0.140625, 0.15625, 0.171875, 0.1875, 0.203125, 0.21875, 0.234375,
    0.25, 0.28125, 0.3125, 0.34375, 0.375, 0.40625, 0.4375, 0.46875,
    0.5, 0.5625, 0.625, 0.6875, 0.75, 0.8125, 0.875, 0.9375,
    1.0, 1.125, 1.25, 1.375, 1.5, 1.625, 1.75, 1.875,
    2.0, 2.25, 2.5, 2.75, 3.0, 3.25, 3.5, 3.75,
    4.0, 4.5, 5.0, 5.5, 6.0, 6.5, 7.0, 7.5,
    8.0, 9.0, 10.0, 11.0, 12.0, 13.0, 14.0, 15.0,
    16.0, 18.0, 20.0, 22.0, 24.0, 26.0, 28.0, 30.0,
    32.0, 36.0, 40.0, 44.0, 48.0, 52.0, 56.0, 60.0,
    64.0, 72.0, 80.0, 88.0, 96.0, 104.0, 112.0, 120.0,
    128.0, 144.0, 160.0, 176.0, 192.0, 208.0, 224.0, 240.0,
    256.0, 288.0, 320.0, 352.0, 384.0, 416.0, 448.0, float('nan'),
    -0.0, -0.001953125, -0.00390625, -0.005859375, -0.0078125, -0.009765625, -0.01171875, -0.013671875,
    -0.015625, -0.017578125, -0.01953125, -0.021484375, -0.0234375, -0.025390625, -0.02734375, -0.029296875,
    -0.03125, -0.03515625, -0.0390625, -0.04296875, -0.046875, -0.05078125, -0.0546875, -0.05859375,
    -0.0625, -0.0703125, -0.078125, -0.0859375, -0.09375, -0.1015625, -0.109375, -0.1171875,
    -0.125, -0.140625, -0.15625, -0.171875, -0.1875, -0.203125, -0.21875, -0.234375,
    -0.25, -0.28125, -0.3125, -0.34375, -0.375, -0.40625, -0.4375, -0.46875,
    -0.5, -0.5625, -0.625, -0.6875, -0.75, -0.8125, -0.875, -0.9375,
    -1.0, -1.125, -1.25, -1.375, -1.5, -1.625, -1.75, -1.875,
    -2.0, -2.25, -2.5, -2.75, -3.0, -3.25, -3.5, -3.75,
    -4.0, -4.5, -5.0, -5.5, -6.0, -6.5, -7.0, -7.5,
    -8.0, -9.0, -10.0, -11.0, -12.0, -13.0, -14.0, -15.0,
    -16.0, -18.0, -20.0, -22.0, -24.0, -26.0, -28.0, -30.0,
    -32.0, -36.0, -40.0, -44.0, -48.0, -52.0, -56.0, -60.0,
    -64.0, -72.0, -80.0, -88.0, -96.0, -104.0, -112.0, -120.0,
    -128.0, -144.0, -160.0, -176.0, -192.0, -208.0, -224.0, -240.0,
    -256.0, -288.0, -320.0, -352.0, -384.0, -416.0, -448.0, float('nan'),
], dtype=np.float64)
assert E4M3FN.shape == (256,) and E4M3FN[0x7e] == 448.0 and E4M3FN[0x01] == 2.0 ** -9 and E4M3FN[0x38] == 1.0
E4M3_MAX = 448.0
_GRID = E4M3FN[:127]                                          # the finite non-negative values, ascending with the code
_MID = (_GRID[:-1] + _GRID[1:]) / 2                           # exact in float64


def encode(y):
    """fp32 values -> codes uint8: round to nearest, ties to the even code, saturated at +-448 (never 0x7f / 0xff); -0.0 and what
    rounds to zero from below keep their sign."""
    y = np.asarray(y, dtype=np.float32)
    a = np.minimum(np.abs(y).astype(np.float64), E4M3_MAX)
    lo = np.searchsorted(_MID, a, side="left")                # first midpoint >= a: codes below it are too small
    tie = (lo < _MID.size) & (_MID[np.minimum(lo, _MID.size - 1)] == a)
    code = np.where(tie & (lo % 2 == 1), lo + 1, lo).astype(np.uint8)      # a tie between lo and lo + 1 goes to the even one
    return code | (np.signbit(y).astype(np.uint8) << 7)


def decode(codes):
    return E4M3FN[np.asarray(codes, dtype=np.uint8)]


def quantize(x):
    """x [rows, C] float32 holding bf16 values (one sequence, one tensor) -> codes uint8 [rows, C], scales float32 [C]."""
    x = np.asarray(x, dtype=np.float32)
    amax = np.abs(x).max(0)
    zero = amax < np.float32(2.0 ** -100)                     # the header's rule: such a column counts as zero
    safe = np.where(zero, np.float32(1), amax)
    inv = np.where(zero, np.float32(1), np.float32(448) / safe).astype(np.float32)
    s = np.where(zero, np.float32(1), safe / np.float32(448)).astype(np.float32)
    return encode((x * inv[None, :]).astype(np.float32)), s


def dequantize(codes, s):
    """s * float(code), the value the kernels use, as an unrounded float64 product."""
    return np.asarray(s, dtype=np.float64)[None, :] * decode(codes)


def dequant_bound(x, s):
    """|s dec - x| <= 2^-4 |x| (1 + 2^-20) + 2^-10 s: half a unit of a 3-bit mantissa relative to the scaled value (whose fp32
    product and scale each carry 2^-24), or half a subnormal step 2^-9 of the scaled value, times the scale."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    return 2.0 ** -4 * x * (1 + 2.0 ** -20) + 2.0 ** -10 * np.asarray(s, dtype=np.float64)[None, :]


def head_major(codes, H):
    """[rows, 64 H] -> [H, rows, 64], the cache layout of one sequence."""
    r = codes.shape[0]
    return np.ascontiguousarray(codes.reshape(r, H, 64).transpose(1, 0, 2))


def attend(q, k8, v8, sK, sV, scale=0.125):
    """One sequence, float64: q [D]; k8, v8 codes [Lk, D]; sK, sV [D] -> softmax_j(scale q . (sK dec k_j)) (sV dec v_j) per head."""
    D = q.shape[0]
    H = D // 64
    k, v = dequantize(k8, sK), dequantize(v8, sV)
    out = np.empty(D)
    for h in range(H):
        c = slice(64 * h, 64 * h + 64)
        s = (k[:, c] @ np.asarray(q, dtype=np.float64)[c]) * scale
        p = np.exp(s - s.max())
        out[c] = (p / p.sum()) @ v[:, c]
    return out


def special_columns(rows, seed=0):
    """float32 [rows, 8] of bf16 values: the columns both test modules quantise -- zeros and magnitudes below 2^-100 (counts as zero); one non-zero; a +-30 outlier among O(1)
    values; values that land on exact ties of the grid after scaling (amax = 448: inv = 1); the subnormal range next to a large
    value; +-amax alone; negative zeros and a tiny negative; plain normal values."""
    rng = np.random.default_rng(seed)
    x = np.zeros((rows, 8), dtype=np.float32)
    x[:, 0] = np.resize(np.array([0.0, 1e-38, -1e-35, -0.0]), rows)      # below 2^-100: the column counts as zero (448 / amax would be inf)
    x[rng.integers(rows), 1] = -0.75
    x[:, 2] = rng.standard_normal(rows)
    x[rng.integers(rows), 2] = 30.0 if seed % 2 else -30.0
    ties = np.array([448.0, 17.0, 19.0, 21.0, 464.0 / 2, 1.5 * 2.0 ** -9, 2.5 * 2.0 ** -9, 2.0 ** -10, 3 * 2.0 ** -10, -208.0, -9.5, 0.0])
    x[:, 3] = np.resize(ties, rows)
    x[:, 4] = np.resize(np.array([448.0] + [m * 2.0 ** -11 for m in range(1, 40)]), rows) * np.resize(np.array([1.0, -1.0]), rows)
    x[:, 5] = np.resize(np.array([3.0, -3.0]), rows)
    x[:, 6] = np.resize(np.array([-0.0, 0.0, -1e-6, 5.0]), rows)
    x[:, 7] = rng.standard_normal(rows)
    import torch
    return torch.from_numpy(x).bfloat16().float().numpy()
