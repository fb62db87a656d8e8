"""TEST INFRASTRUCTURE -- float64 restatement of the attention entry points of libdwamd.so (csrc/attention.hip), the per-row error
metric, and the inputs / closed-form expectations of the mask census, for tests/test_attention_edges*.py.

Unlike oracle/ref_ops.py, which rounds P, dS and the outputs to bf16 where the kernels do, nothing is rounded here: the inputs are the
bf16 tensors the kernels read (token-major [B * L, H * 64]), every product and sum is float64 on whatever device the inputs live on.
The product never imports this module."""
import math

import torch

SCALE = 0.125
NAN16 = 0x7FC1          # bf16 NaN bit pattern of the guard elements (a quiet NaN no kernel produces: payload 1)
NAN32 = 0x7FC00001      # fp32 one


# ---- float64 attention -------------------------------------------------------------------------------------------------------
def _heads(t, B, L, H):
    return t.reshape(B, L, H, 64).permute(0, 2, 1, 3).double()


def _rows(t, B, L, H):
    return t.permute(0, 2, 1, 3).reshape(B * L, H * 64)


def visible(Lq, Lk, causal, device="cpu"):
    """bool [Lq, Lk]: query i may see key j.  causal 0 none, 1 j <= i, 2 bottom-right aligned j <= i + Lk - Lq."""
    m = torch.ones(Lq, Lk, dtype=torch.bool, device=device)
    if int(causal) == 0:
        return m
    return m.tril(Lk - Lq if int(causal) == 2 else 0)


def _unpitch(t, B, Lk, pitch):
    if pitch is None or pitch == Lk:
        return t
    return t.reshape(B, pitch, -1)[:, :Lk].reshape(B * Lk, -1)


def _probs(q, k, B, H, Lq, Lk, causal, scale):
    s = (_heads(q, B, Lq, H) @ _heads(k, B, Lk, H).transpose(-1, -2)) * scale
    s = s.masked_fill(~visible(Lq, Lk, causal, s.device), float("-inf"))
    lse = torch.logsumexp(s, -1)
    return torch.exp(s - lse[..., None]), lse


def attn_fwd(q, k, v, B, H, Lq, Lk, causal, scale=SCALE, kv_batch_rows=None):
    """-> o float64 [B * Lq, H * 64], lse float64 [B, H, Lq]."""
    k, v = _unpitch(k, B, Lk, kv_batch_rows), _unpitch(v, B, Lk, kv_batch_rows)
    p, lse = _probs(q, k, B, H, Lq, Lk, causal, scale)
    return _rows(p @ _heads(v, B, Lk, H), B, Lq, H), lse


def attn_bwd(q, k, v, do, B, H, Lq, Lk, causal, scale=SCALE):
    """-> dq, dk, dv float64, token-major, from this module's own forward: dS = P * (dP - delta) with
    delta_i = sum_j P_ij dP_ij (= dO_i . o_i with o = P v).  Summed over the keys like that, a query with one visible key has
    dS = 0 exactly, as it must."""
    p, _ = _probs(q, k, B, H, Lq, Lk, causal, scale)
    qh, kh, vh, doh = _heads(q, B, Lq, H), _heads(k, B, Lk, H), _heads(v, B, Lk, H), _heads(do, B, Lq, H)
    dp = doh @ vh.transpose(-1, -2)
    ds = p * (dp - (p * dp).sum(-1, keepdim=True))
    return (_rows((ds @ kh) * scale, B, Lq, H), _rows((ds.transpose(-1, -2) @ qh) * scale, B, Lk, H),
            _rows(p.transpose(-1, -2) @ doh, B, Lk, H))


# ---- the metric --------------------------------------------------------------------------------------------------------------
def row_err(x, ref, H):
    """max over the (row, head) 64-vectors of ||x - ref|| / max(||ref row||, rms), rms = root mean square of all row norms of ref.
    The floor keeps rows whose reference is (nearly) zero -- dq of causal row 0 -- from dividing by nothing, and judges the small
    late rows of a causal output on the scale of the tensor.  An identically zero `ref` has no scale: see zero_ref()."""
    x, ref = x.double().reshape(-1, H, 64), ref.double().reshape(-1, H, 64)
    n = ref.norm(dim=-1)
    rms = n.pow(2).mean().sqrt()
    return ((x - ref).norm(dim=-1) / torch.maximum(n, rms)).max().item()


def zero_ref(ref):
    """dq and dk are identically zero when every query sees one key (Lk == 1, or causal == 1 with Lq == 1)."""
    return not bool(ref.any())


ZERO_ABS = 1e-4   # bound on max|x| against an identically zero reference: dP = dO.v and delta = dO.o cancel exactly in exact
                  # arithmetic; what a kernel leaves is the fp32 ordering difference of two 64-term dot products of size ~8,
                  # 64 * 6e-8 * 8 = 3e-5, before the 0.125 scale


def check(name, x, ref, H, bound):
    """The per-row comparison every test makes: finite, then row_err <= bound (max|x| <= ZERO_ABS against a zero reference).
    -> the figure, for the callers that print it."""
    assert torch.isfinite(x.float()).all(), f"{name}: non-finite values"
    if zero_ref(ref):
        e = x.double().abs().max().item()
        assert e <= ZERO_ABS, f"{name}: max|x| = {e:.3e} against a zero reference"
        return e
    e = row_err(x, ref, H)
    assert math.isfinite(e) and e <= bound, f"{name}: row_err {e:.3e} > {bound:.3e}"
    return e


# ---- shapes ------------------------------------------------------------------------------------------------------------------
# (B, H, Lq, Lk, causal, factor on q and k)
SWEEP = [
    (1, 1, 1, 1, 0, 1.0),
    (2, 2, 33, 65, 0, 1.0),
    (1, 2, 129, 129, 1, 1.0),
    (1, 1, 65, 193, 0, 1.0),
    (1, 1, 130, 70, 1, 1.0),
    (1, 1, 70, 130, 1, 1.0),
    (1, 1, 5, 200, 1, 1.0),
    (2, 1, 257, 385, 0, 1.0),
    (1, 1, 447, 447, 1, 1.0),
    (3, 3, 100, 200, 0, 1.0),      # 9 forward / dQ workgroups, 18 dK/dV workgroups
    (1, 5, 300, 300, 1, 1.0),      # 15 workgroups
    (1, 17, 64, 64, 0, 1.0),       # 17 workgroups
    (1, 1, 320, 320, 0, 3.0),      # peaked rows
    (1, 1, 65, 129, 1, 4.0),
]
SWEEP_BR = [(2, 1, 70, 200, 200), (1, 2, 130, 447, 448)]      # forward only, causal = 2: (B, H, Lq, Lk, pitch)
SWEEP_ONE = [9, 511, 512, 1500]                                # forward only, one query, B = 3, H = 2: Lk


def sweep_inputs(B, H, Lq, Lk, qk_factor=1.0, kv_batch_rows=None, seed=0, device="cpu"):
    """Unit-scale q / k / v as column slices of one fused [rows, 3 * H * 64] buffer, as the engine has them, and dO.  Drawn on the
    CPU from `seed` whatever the device, so the CPU and GPU tests judge the same numbers."""
    D, kr = H * 64, Lk if kv_batch_rows is None else kv_batch_rows
    g = torch.Generator().manual_seed(1000 + seed)
    x = torch.randn(B * max(Lq, kr), 3 * D, generator=g)
    x[:, :2 * D] *= qk_factor
    qkv = x.bfloat16().to(device)
    do = torch.randn(B * Lq, D, generator=g).bfloat16().to(device)
    return qkv[:B * Lq, :D], qkv[:B * kr, D:2 * D], qkv[:B * kr, 2 * D:], do


# ---- mask census -------------------------------------------------------------------------------------------------------------
# k = 0: every score is 0, so lse_i = log(n_i) with n_i the number of keys query i may see.  v is one-hot: key j has its 1 at
# column j % 64 in head 0 and at column (j // 64) % 64 in head 1, so o_i[d] * n_i is the number of visible keys in each residue
# class / each 64-block: WHICH keys a query saw, as integers.  Rows of a padded cache behind Lk hold k = 0, v = 1e4.
CENSUS_H = 2
CENSUS_PAD = 1.0e4


def census_kv(B, Lk, pitch=None, device="cpu"):
    pitch = Lk if pitch is None else pitch
    j = torch.arange(pitch)
    v = torch.zeros(pitch, 128)
    v[j, j % 64] = 1.0
    v[j, 64 + (j // 64) % 64] = 1.0
    v[Lk:] = CENSUS_PAD
    v = v.repeat(B, 1).bfloat16().to(device)
    return torch.zeros_like(v), v


def census_q(rows, seed=0, device="cpu"):
    g = torch.Generator().manual_seed(2000 + seed)
    return torch.randn(rows, 128, generator=g).bfloat16().to(device)


def census_expect(Lq, Lk, causal):
    """-> n int64 [Lq], counts int64 [Lq, 128] (both heads), in closed form from the mask rule."""
    vis = visible(Lq, Lk, causal).long()
    j = torch.arange(Lk)
    onehot = torch.zeros(Lk, 128, dtype=torch.long)
    onehot[j, j % 64] = 1
    onehot[j, 64 + (j // 64) % 64] = 1
    return vis.sum(1), vis @ onehot


def census_counts(o, n):
    """Integer counts out of an output row block o [Lq, 128] and the visible-key numbers n [Lq].  P and o are each rounded to bf16
    at most (relative 2 * 2^-9 together) and the counts here are at most 64: the product is off by at most 0.25."""
    return torch.round(o.double().cpu() * n.double()[:, None]).long()


def census_lse_bound(n):
    """Half the smallest move of lse a wrongly visible (or hidden) key makes: 0.5 * log(1 + 1 / max n)."""
    return 0.5 * math.log1p(1.0 / int(n.max()))


def census_check(name, o, lse, Lq, Lk, causal, counts=True):
    """o [Lq, 128] and lse [2, Lq] (or None) of ONE batch entry against the closed form."""
    n, want = census_expect(Lq, Lk, causal)
    assert torch.isfinite(o.float()).all(), f"{name}: non-finite output"
    if counts:
        got = census_counts(o, n)
        bad = (got != want).any(1).nonzero().flatten().tolist()
        assert not bad, f"{name}: visible-key counts differ at queries {bad[:8]} (first: got {got[bad[0]].tolist()}, want {want[bad[0]].tolist()})"
    if lse is not None:
        d = (lse.double().cpu() - n.double().log()[None]).abs()
        assert d.max().item() <= census_lse_bound(n), f"{name}: |lse - log n| = {d.max().item():.3e} at query {int(d.max(0).values.argmax())}"


TILE_LQ = [1, 31, 32, 33, 64, 65, 127, 128, 129]
TILE_LK = [1, 63, 64, 65, 127, 128, 129, 193]
BR_CASES = [(1, 2, 2, 8), (3, 6, 37, 48), (1, 33, 64, 64), (1, 65, 129, 136), (1, 130, 447, 448)]     # (B, Lq, Lk, pitch), causal = 2
ONE_LK = [1, 7, 8, 9, 31, 32, 33, 511, 512, 513, 1500, 1535, 1536, 1537]
ONE_LK_LSE_ONLY = [8191, 8192, 8193]       # head 0 counts pass 64 there
ONE_CAUSAL1_LK = [1, 9, 600, 8193]
VARLEN_LENS = [1, 32, 33, 64, 65, 128, 129]
VARLEN_LK = 65
