"""TEST INFRASTRUCTURE -- float64 restatement of the token step's attention with its projection inside (`attn_decode_proj_kernel`,
csrc/decode.hip, reached alone through dw_decode_attn_proj), its inputs, the closed forms of its census, the table of the kernel
instantiations a case reaches, and a float64 decoder pass built from the same statement, for tests/test_decode_edges*.py.

Nothing is rounded here: the inputs are the bf16 / f32 tensors the kernel reads, every product and sum is float64 on whatever device
the inputs live on.  `composed` is the same operation out of `RefOps.layernorm_fwd`, `gemm` and `attn_fwd`, which round where the
kernel rounds (the normalised row, q / k / v, P and o): its distance from float64 is the yardstick e_ref of the GPU tests.
The product never imports this module."""
import functools
import math

import torch

from attention_restatement import CENSUS_PAD, row_err          # noqa: F401  (row_err: the metric of every edge suite)

SCALE = 0.125
EPS = 1e-5
WIDTHS = (384, 512, 768, 1024, 1280)
MAX_KEYS = 8192


# ---- which kernel a case reaches -----------------------------------------------------------------------------------------------
def instantiation(mode, x_dtype, D):
    """-> (MODE, XBF, NI) of attn_decode_proj_kernel<MODE, XBF, NI>, or None where dw_decode_attn_proj refuses."""
    if mode not in (0, 1) or x_dtype not in (torch.float32, torch.bfloat16) or D not in WIDTHS:
        return None
    return int(mode), x_dtype == torch.bfloat16, D // 64


INSTANTIATIONS = frozenset((m, xb, D // 64) for m in (0, 1) for xb in (False, True) for D in WIDTHS)       # the twenty


# ---- the float64 statement -----------------------------------------------------------------------------------------------------
def layer_norm(x, gamma, beta, eps=EPS):
    x = x.double()
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * gamma.double() + beta.double()


def attend(q, k, v, H, scale=SCALE):
    """q [B, D], k / v [B, Lk, D] -> softmax(scale q.k) v per head, [B, D]; all float64."""
    B, Lk, D = k.shape
    qh = q.reshape(B, H, 1, 64)
    kh, vh = (t.reshape(B, Lk, H, 64).permute(0, 2, 1, 3) for t in (k, v))
    s = (qh @ kh.transpose(-1, -2)) * scale
    s = s - s.amax(-1, keepdim=True)
    p = torch.exp(s)
    return ((p / p.sum(-1, keepdim=True)) @ vh).reshape(B, D)


def _old_keys(t, B, kv_rows, n):
    """rows [0, n) of every sequence out of a 2-D [B * kv_rows, D] view (any row pitch)."""
    return t.reshape(B, kv_rows, t.shape[-1])[:, :n]


def decode_attn_proj(mode, x, ln_g, ln_b, w, bias, k, v, B, H, Lk, kv_rows=None, eps=EPS, scale=SCALE):
    """-> o [B, D], k_new, v_new [B, D] (None in mode 0), float64.  mode 1: w [3D, D] stacks q | k | v, the softmax runs over the
    Lk - 1 rows of k / v in front of row t = Lk - 1 and the new key; k_new | v_new is the cache row t that results."""
    D = H * 64
    kv_rows = Lk if kv_rows is None else kv_rows
    proj = layer_norm(x[:B], ln_g, ln_b, eps) @ w.double().t() + bias.double()
    nold = Lk - 1 if mode == 1 else Lk
    k3, v3 = _old_keys(k, B, kv_rows, nold).double(), _old_keys(v, B, kv_rows, nold).double()
    if mode == 0:
        return attend(proj, k3, v3, H, scale), None, None
    q, kn, vn = proj[:, :D], proj[:, D:2 * D], proj[:, 2 * D:]
    return attend(q, torch.cat([k3, kn[:, None]], 1), torch.cat([v3, vn[:, None]], 1), H, scale), kn, vn


def composed(ref, mode, x, ln_g, ln_b, w, bias, k, v, B, H, Lk, kv_rows=None, eps=EPS, scale=SCALE):
    """The same operation out of `ref`'s layernorm_fwd, gemm and attn_fwd (oracle.ref_ops.RefOps: bf16 where the kernel has bf16)
    -> o, k_new, v_new in ref.lowp."""
    D = H * 64
    kv_rows = Lk if kv_rows is None else kv_rows
    ln = ref.layernorm_fwd(x[:B], ln_g, ln_b, eps, save_stats=False)[0]
    proj = ref.gemm(ln, w, bias=bias)
    nold = Lk - 1 if mode == 1 else Lk
    k3, v3 = _old_keys(k, B, kv_rows, nold).to(proj.dtype), _old_keys(v, B, kv_rows, nold).to(proj.dtype)
    kn = vn = None
    q = proj
    if mode == 1:
        q, kn, vn = proj[:, :D], proj[:, D:2 * D], proj[:, 2 * D:]
        k3, v3 = torch.cat([k3, kn[:, None]], 1), torch.cat([v3, vn[:, None]], 1)
    o, _ = ref.attn_fwd(q.contiguous(), k3.reshape(B * Lk, D), v3.reshape(B * Lk, D), B, H, 1, Lk, 0, scale)
    return o, kn, vn


def vec_err(x, ref):
    """row_err with the whole row as the vector (logits rows, K | V cache rows): max over rows of ||x - ref|| / max(||ref row||, rms)."""
    x, ref = x.double().reshape(-1, ref.shape[-1]), ref.double().reshape(-1, ref.shape[-1])
    n = ref.norm(dim=-1)
    return ((x - ref).norm(dim=-1) / torch.maximum(n, n.pow(2).mean().sqrt())).max().item()


# ---- inputs of the boundary sweep ----------------------------------------------------------------------------------------------
SWEEP_LK = (1, 2, 9, 65, 513, 1500)
SWEEP_B = (1, 3)
SPIKE = 6.0          # factor on the cached keys of the spiked-score cases: scores of standard deviation ~6, a handful of keys carry P
SWEEP_SPIKED = ((384, 65), (768, 513), (1280, 1500))          # (D, Lk), both modes, both dtypes, B = 3, padded pitch
PITCH_PAD = 64       # elements: the engine's kv_row_pad


def sweep_cases():
    """(D, mode, x_dtype, Lk, B, padded, spiked): every width x mode x stream dtype x key count x batch x pitch, then the spiked ones."""
    out = [(D, mode, dt, Lk, B, padded, False) for D in WIDTHS for mode in (0, 1) for dt in (torch.float32, torch.bfloat16)
           for Lk in SWEEP_LK for B in SWEEP_B for padded in (False, True)]
    out += [(D, mode, dt, Lk, 3, True, True) for D, Lk in SWEEP_SPIKED for mode in (0, 1) for dt in (torch.float32, torch.bfloat16)]
    return out


@functools.lru_cache(maxsize=None)
def sweep_params(D, device="cpu"):
    """ln_g, ln_b f32 [D]; w bf16 [3D, D] at 1 / sqrt(D) scale; bias f32 [3D].  Mode 0 takes the first D rows of w and bias."""
    g = torch.Generator().manual_seed(4000 + D)
    ln_g = (1.0 + 0.25 * torch.randn(D, generator=g)).to(device)
    ln_b = (0.25 * torch.randn(D, generator=g)).to(device)
    w = (torch.randn(3 * D, D, generator=g) / math.sqrt(D)).bfloat16().to(device)
    bias = (0.5 * torch.randn(3 * D, generator=g)).to(device)
    return ln_g, ln_b, w, bias


def sweep_case_inputs(D, mode, x_dtype, Lk, B, padded, spiked=False, device="cpu"):
    """-> x [B, D] (N(0, 1) plus a per-row offset), kv bf16 [B * kv_rows, pitch] with K | V in columns [0, 2D) of the rows
    [0, n_old) of every sequence and NaN everywhere else, kv_rows.  Drawn on `device` from a seed of the case."""
    g = torch.Generator(device=device).manual_seed(5000 + D + 7 * Lk + 100003 * B + 3 * mode + 5 * int(padded) + 11 * int(spiked)
                                                   + 13 * int(x_dtype == torch.bfloat16))
    rn = lambda *shape: torch.randn(*shape, generator=g, device=device)
    x = (rn(B, D) + 2.0 * rn(B, 1)).to(x_dtype)
    kv_rows, pitch = Lk + 2, 2 * D + (PITCH_PAD if padded else 0)
    nold = Lk - 1 if mode == 1 else Lk
    kv = torch.full((B, kv_rows, pitch), float("nan"), dtype=torch.bfloat16, device=device)
    hist = rn(B, nold, 2 * D)
    if spiked:
        hist[..., :D] *= SPIKE
    kv[:, :nold, :2 * D] = hist.bfloat16()
    return x, kv.reshape(B * kv_rows, pitch), kv_rows


# ---- census ------------------------------------------------------------------------------------------------------------------------
# Zero gamma makes the normalised row beta, zero weights make q / k / v their biases, cached K = 0 and a zero k bias make every score
# equal: P is uniform whatever x, beta and the q bias are.  V is one-hot: key j has its 1 at column j % 64 in the even heads and at
# column (j // 64) % 64 in the odd ones (the new key of mode 1 through the v bias), so o * Lk is the number of keys in each residue
# class / each 64-block: WHICH keys entered the sum, as integers.  The kernel's sums are then sums of ones (exact in fp32), its
# denominator is Lk, and o = bf16(count / Lk) bit for bit.  Cache rows from Lk on (in mode 1: from t on) and the pad columns of a
# padded pitch hold CENSUS_PAD in K and in V.
CENSUS_LK = (1, 2, 7, 8, 9, 63, 64, 65, 127, 129, 511, 512, 513, 1023, 1025, 8191, 8192)
CENSUS_WIDE = (1280, (1, 513, 8192))
CENSUS_GUARD_ROWS = 3


def census_onehot(j, H):
    """float32 [len(j), 64 * H]: the V rows of the keys j."""
    j = torch.as_tensor(j, dtype=torch.long).reshape(-1)
    even = torch.nn.functional.one_hot(j % 64, 64).float()
    odd = torch.nn.functional.one_hot((j // 64) % 64, 64).float()
    return torch.stack([even if h % 2 == 0 else odd for h in range(H)], 1).reshape(j.numel(), H * 64)


def census_counts(Lk, H):
    """int64 [64 * H]: how many of the keys 0 .. Lk - 1 have their 1 in each column -- in closed form, no key is enumerated."""
    c = torch.arange(64)
    even = Lk // 64 + (c < Lk % 64).long()
    odd = sum(torch.clamp(Lk - 64 * (c + 64 * wrap), 0, 64) for wrap in range((Lk + 4095) // 4096))
    return torch.stack([even if h % 2 == 0 else odd for h in range(H)]).reshape(64 * H)


def census_expect(Lk, H):
    """bf16 [64 * H]: the output row, bit for bit (fp32 quotient of two integers, rounded once)."""
    return (census_counts(Lk, H).float() / float(Lk)).bfloat16()


@functools.lru_cache(maxsize=None)
def _census_zero_weights(D, device):
    return torch.zeros(3 * D, D, dtype=torch.bfloat16, device=device)


def census_inputs(mode, D, B, Lk, padded, x_dtype=torch.float32, device="cpu"):
    """-> dict(x, ln_g, ln_b, w, bias, kv, kv_rows): see the comment above."""
    H = D // 64
    g = torch.Generator().manual_seed(6000 + Lk + 3 * mode + 7 * B)
    x = (3.0 * torch.randn(B, D, generator=g)).to(x_dtype).to(device)
    ln_b = torch.randn(D, generator=g).to(device)
    bias = torch.zeros(3 * D if mode == 1 else D)
    bias[:D] = torch.randn(D, generator=g)
    nold = Lk - 1 if mode == 1 else Lk
    if mode == 1:
        bias[2 * D:] = census_onehot([nold], H)[0]
    kv_rows, pitch = Lk + CENSUS_GUARD_ROWS, 2 * D + (PITCH_PAD if padded else 0)
    kv = torch.full((B, kv_rows, pitch), CENSUS_PAD, dtype=torch.bfloat16, device=device)
    kv[:, :nold, :D] = 0.0
    kv[:, :nold, D:2 * D] = census_onehot(torch.arange(nold), H).bfloat16().to(device)
    w = _census_zero_weights(D, str(device))
    return dict(x=x, ln_g=torch.zeros(D, device=device), ln_b=ln_b, w=w if mode == 1 else w[:D], bias=bias.to(device),
                kv=kv.reshape(B * kv_rows, pitch), kv_rows=kv_rows)


# ---- P is rounded to bf16 in front of the PV product -----------------------------------------------------------------------------
# Two keys of one head with opposite values: key 0 scores 0 (P = 1, exact), key 1 scores a little less, so that its P = 2^s sits
# between two bf16 numbers near 1 (spacing 2^-8), well away from the midpoint.  o = (1 - bf16(P)) / (1 + P) in the column where
# v = (+1, -1): the difference keeps the rounding of P and nothing else -- with P left unrounded it would be (1 - P) / (1 + P).
P_ROUND_K = -0.0222          # key 1, element 0 (q is 1 there, through the q bias): s = scale * log2(e) * bf16(P_ROUND_K)


def p_rounding_expect(scale=SCALE):
    """-> (o with P rounded, o with P unrounded), float64, in column 0 of head 0."""
    k1 = torch.tensor(P_ROUND_K).bfloat16().double().item()
    p = 2.0 ** (scale * 1.4426950408889634 * k1)
    pb = torch.tensor(p).bfloat16().double().item()
    assert min(abs(p - (pb + d)) for d in (2.0 ** -9, -2.0 ** -9)) > 2.0 ** -11, "P is too close to a bf16 midpoint"
    return (1.0 - pb) / (1.0 + p), (1.0 - p) / (1.0 + p)


def p_rounding_inputs(D, device="cpu"):
    """Mode 0 inputs, B = 1, Lk = 2: zero gamma / weights, q bias = e_0 in head 0, K | V as described above."""
    bias = torch.zeros(D)
    bias[0] = 1.0
    kv = torch.zeros(2, 2 * D)
    kv[1, 0] = P_ROUND_K
    kv[0, D], kv[1, D] = 1.0, -1.0
    return dict(x=torch.randn(1, D, generator=torch.Generator().manual_seed(7)).to(device), ln_g=torch.zeros(D, device=device),
                ln_b=torch.zeros(D, device=device), w=_census_zero_weights(D, str(device))[:D], bias=bias.to(device),
                kv=kv.bfloat16().to(device), kv_rows=2)


# ---- a whole decoder pass (token step) from the statement above ------------------------------------------------------------------
def _f64(sd, name):
    return sd[name].double()


def cross_kv(sd, dims, enc, B):
    """Per decoder layer the static K | V of the encoder states enc [B * max_src, D] -> list of float64 [B * max_src, 2D]."""
    out = []
    for i in range(dims.dec_layers):
        p = f"model.decoder.layers.{i}.encoder_attn"
        e = enc.double()
        out.append(torch.cat([e @ _f64(sd, f"{p}.k_proj.weight").t(),
                              e @ _f64(sd, f"{p}.v_proj.weight").t() + _f64(sd, f"{p}.v_proj.bias")], 1))
    return out


def decode_pass(sd, dims, ids, t, self_kv, cross):
    """One token step in float64: ids int64 [B, 1] at position t; self_kv[l] [B * max_len, 2D] whose rows < t of every sequence
    are the history (others are not read); cross[l] from cross_kv() -> logits [B, vocab], and per layer the cache row t [B, 2D]."""
    D, H, B = dims.d_model, dims.heads, ids.shape[0]
    x = _f64(sd, "model.decoder.embed_tokens.weight")[ids[:, 0]] + _f64(sd, "model.decoder.embed_positions.weight")[t]
    rows = []
    for i in range(dims.dec_layers):
        p = f"model.decoder.layers.{i}"
        sa, ca = f"{p}.self_attn", f"{p}.encoder_attn"
        w = torch.cat([_f64(sd, f"{sa}.{n}_proj.weight") for n in "qkv"])
        bias = torch.cat([_f64(sd, f"{sa}.q_proj.bias"), torch.zeros(D, dtype=torch.float64, device=x.device), _f64(sd, f"{sa}.v_proj.bias")])
        kv = self_kv[i]
        o, kn, vn = decode_attn_proj(1, x, _f64(sd, f"{sa}_layer_norm.weight"), _f64(sd, f"{sa}_layer_norm.bias"), w, bias,
                                     kv[:, :D], kv[:, D:], B, H, t + 1, kv_rows=kv.shape[0] // B)
        rows.append(torch.cat([kn, vn], 1))
        x = x + o @ _f64(sd, f"{sa}.out_proj.weight").t() + _f64(sd, f"{sa}.out_proj.bias")
        o, _, _ = decode_attn_proj(0, x, _f64(sd, f"{ca}_layer_norm.weight"), _f64(sd, f"{ca}_layer_norm.bias"),
                                   _f64(sd, f"{ca}.q_proj.weight"), _f64(sd, f"{ca}.q_proj.bias"), cross[i][:, :D], cross[i][:, D:],
                                   B, H, dims.max_src)
        x = x + o @ _f64(sd, f"{ca}.out_proj.weight").t() + _f64(sd, f"{ca}.out_proj.bias")
        h = layer_norm(x, _f64(sd, f"{p}.final_layer_norm.weight"), _f64(sd, f"{p}.final_layer_norm.bias"))
        a = h @ _f64(sd, f"{p}.fc1.weight").t() + _f64(sd, f"{p}.fc1.bias")
        a = 0.5 * a * (1.0 + torch.erf(a * 0.7071067811865476))
        x = x + a @ _f64(sd, f"{p}.fc2.weight").t() + _f64(sd, f"{p}.fc2.bias")
    h = layer_norm(x, _f64(sd, "model.decoder.layer_norm.weight"), _f64(sd, "model.decoder.layer_norm.bias"))
    return h @ _f64(sd, "model.decoder.embed_tokens.weight").t(), rows


# ---- whole-pass cases of the GPU test ----------------------------------------------------------------------------------------------
PASS_FFN, PASS_VOCAB, PASS_SRC, PASS_MAX_LEN = 256, 1030, 72, 24
PASS_KEYS = (0, 4, 8, 12)                                         # dw_debug_set key 7
PASS_BT = ((1, 0), (3, 5), (3, PASS_MAX_LEN - 1))
PASS_BT_384 = ((33, 1), (65, 1))                                  # past the rows <= 32 / <= 64 fusion switches of decode_pass


def pass_launches(D, key, B, t, rows_pass=False):
    """-> (self-attention fused, cross-attention fused): which of a layer's two attentions of a token step run in
    attn_decode_proj_kernel under dw_debug_set(7, key) -- the rule of decode_pass (csrc/decode.hip), restated."""
    ok = D in WIDTHS
    return (ok and not rows_pass and not key & 4 and t + 1 <= MAX_KEYS, ok and not key & 8 and PASS_SRC <= MAX_KEYS)
