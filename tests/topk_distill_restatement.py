"""Float64 restatements of the stored top-k teacher targets (include/dwamd.h, "Stored top-k teacher targets") and of the loss over them
(csrc/topk_distill.hip): plain formulas on the inputs as the kernels see them (bf16 / fp32 values widened exactly), no rounding point
shared with the kernels or with distil_whisper_amd/topk_distill.py.  The dense loss is tests/training_restatement.py's, unchanged."""
import numpy as np
import torch

import training_restatement as tr
from training_restatement import distill_loss as dense_loss      # noqa: F401  (the dense limit and the bucket bound compare with it)

FLT_MIN = float(np.finfo(np.float32).tiny)      # the clamp of the student's tail sum (dwamd.h)


def select(z, k):
    """z float64 numpy [rows, V] -> int64 [rows, k]: the k largest, equal values to the lower column, ordered by value descending
    then column ascending (-0 == +0 as numbers)."""
    rows, V = z.shape
    cols = np.arange(V)
    return np.stack([np.lexsort((cols, -(z[r] + 0.0)))[:k] for r in range(rows)])


def targets(logits, V, T, k):
    """-> idx int64 [rows, k], logp float64 [rows, k], rest float64 [rows] (numpy).  T as the kernel receives it (a float)."""
    z = logits[:, :V].detach().double().cpu().numpy()
    Td = tr.f32_as_double(T)
    idx = select(z, k)
    zt = z / Td
    m = zt.max(-1, keepdims=True)
    lse = m + np.log(np.exp(zt - m).sum(-1, keepdims=True))
    lp = zt - lse
    member = np.zeros(z.shape, dtype=bool)
    np.put_along_axis(member, idx, True, axis=1)
    rest = np.where(member, 0.0, np.exp(lp)).sum(-1)
    return idx, np.take_along_axis(lp, idx, axis=1), rest


def loss(s, idx, logp, rest, labels, V, T, ce_w, kl_w, grad_scale):
    """-> row_ce, row_kl [rows] (0 in the rows the label excludes; row_kl in the dense restatement's units: T^2 enters with the mean),
    losses [4], gradient [rows, V] -- the returns of tr.distill_loss.  idx / logp / rest: tensors or numpy; only rows with
    label >= 0 are looked at."""
    zs = tr._d(s)[:, :V]
    rows = zs.shape[0]
    T = tr.f32_as_double(T)
    idx = torch.as_tensor(np.asarray(idx)).long()
    logp, rest = torch.as_tensor(np.asarray(logp)).double(), torch.as_tensor(np.asarray(rest)).double()
    ce_ok, kl_ok = labels != -100, labels >= 0
    n_ce, n_kl = int(ce_ok.sum()), int(kl_ok.sum())
    logp1 = zs - tr._lse(zs)
    m = zs.max(-1, keepdim=True).values
    e = torch.exp((zs - m) / T)
    Z = e.sum(-1, keepdim=True)
    logq = (zs - m) / T - torch.log(Z)
    row_kl = torch.zeros(rows, dtype=torch.float64)
    gk = torch.zeros(rows, V, dtype=torch.float64)
    for r_ in torch.nonzero(kl_ok).flatten().tolist():
        K = idx[r_]
        p, lp, rr = torch.exp(logp[r_]), logp[r_], float(rest[r_])
        member = torch.zeros(V, dtype=torch.bool)
        member[K] = True
        S = max(float(e[r_][~member].sum()), FLT_MIN)
        kl = float((p * (lp - logq[r_, K])).sum())
        if rr > 0:
            kl += rr * (np.log(rr) - (np.log(S) - float(torch.log(Z[r_, 0]))))
        row_kl[r_] = kl
        g = e[r_] * (1.0 / Z[r_, 0] - (rr / S if rr > 0 else 0.0))
        g[K] = e[r_, K] / Z[r_, 0] - p
        gk[r_] = g
    onehot = torch.zeros_like(zs)
    has = ce_ok & (labels >= 0) & (labels < V)      # (a label outside [0, V) other than -100 counts in the mean and has no term)
    ii = torch.nonzero(has).flatten()
    onehot[ii, labels[ii]] = 1.0
    row_ce = -(logp1 * onehot).sum(-1)
    nan = float("nan")
    ce = row_ce.sum().item() / n_ce if n_ce else nan
    kl = row_kl.sum().item() / n_kl * T * T if n_kl else nan
    losses = torch.tensor([ce, kl, ce_w * ce + kl_w * kl, float(n_ce)], dtype=torch.float64)
    grad = torch.zeros(rows, V, dtype=torch.float64)
    if n_ce:
        grad += (grad_scale * ce_w / n_ce) * (torch.exp(logp1) - onehot) * has[:, None]
    if n_kl:
        grad += (grad_scale * kl_w * T / n_kl) * gk * kl_ok[:, None]
    return row_ce, row_kl, losses, grad


def tie_rows(V, k, seed=0):
    """bf16 rows [5, V] with planted ties: a run of equal values straddling the k-th place (its members spread over the row), all
    columns equal, the maximum repeated (2 k times), a Gaussian row with signed zeros, a Gaussian row."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * V + k)
    z = (2.0 * torch.randn(5, V, generator=g)).to(torch.bfloat16)
    perm = torch.randperm(V, generator=g)
    a = max(0, k - 2)
    z[0, perm[:a]] = 9.0                                 # k - 2 columns above the run
    z[0, perm[a:a + min(V - a, 7)]] = 8.5                # the run: 7 equal values over places k - 1 ...
    z[1] = -1.25
    z[2, perm[:min(V, 2 * k)]] = 11.0
    z[3, perm[:min(V, 6)]] = torch.tensor([0.0, -0.0, 0.0, -0.0, 0.0, -0.0])[:min(V, 6)].to(torch.bfloat16)
    z[3] = torch.minimum(z[3], torch.zeros_like(z[3]))   # the zeros are the row's maximum: signed zeros tie
    return z
