"""Offline distillation from stored top-k teacher log-probabilities: the container, and torch statements of the two kernels.

The format is stated once, in include/dwamd.h ("Stored top-k teacher targets"): per label position the k columns with the largest
teacher logit (equal values to the lower column; value descending, then column ascending), their log-probabilities at temperature T
and the probability mass of all other columns, summed term by term.  The kernels are csrc/topk_distill.hip (`dw_logits_topk`,
`dw_distill_loss_topk`, `dw_distill_loss_topk_w`); the functions here are what ops without them run (oracle.ref_ops, the CPU) and what
the tests hold the kernels against, next to the float64 statement tests/topk_distill_restatement.py.
"""
import numbers

import torch

MAX_K = 64
FLT_MIN = 1.1754943508222875e-38       # 2^-126: the clamp of the student's tail sum (dwamd.h)


def check_k(k, vocab=None):
    if not isinstance(k, numbers.Integral) or not 1 <= int(k) <= MAX_K:
        raise ValueError(f"top-k teacher targets hold 1 to {MAX_K} columns per position, got k = {k!r}")
    if vocab is not None and int(k) >= int(vocab):
        raise ValueError(f"k = {k} must be below the vocabulary size {vocab}")
    return int(k)


class TeacherTopK:
    """Stored teacher targets of one batch: idx int32 [B, Td, k], logp float32 [B, Td, k], rest float32 [B, Td], the temperature
    they were made at and the vocabulary size.  Plain tensors and numbers: `as_dict()` is what a dataset column or `torch.save`
    carries, `from_dict()` brings it back."""

    def __init__(self, idx, logp, rest, temperature, vocab):
        if not (torch.is_tensor(idx) and torch.is_tensor(logp) and torch.is_tensor(rest)):
            raise ValueError("TeacherTopK: idx, logp and rest are tensors")
        if idx.dtype != torch.int32 or logp.dtype != torch.float32 or rest.dtype != torch.float32:
            raise ValueError(f"TeacherTopK: idx int32, logp float32, rest float32; got {idx.dtype}, {logp.dtype}, {rest.dtype}")
        if idx.dim() != 3 or logp.shape != idx.shape or tuple(rest.shape) != tuple(idx.shape[:2]):
            raise ValueError(f"TeacherTopK: idx and logp [B, Td, k], rest [B, Td]; got {tuple(idx.shape)}, {tuple(logp.shape)}, "
                             f"{tuple(rest.shape)}")
        if not (idx.device == logp.device == rest.device):
            raise ValueError("TeacherTopK: the three tensors live on one device")
        if not isinstance(vocab, numbers.Integral) or int(vocab) < 2:
            raise ValueError(f"TeacherTopK: vocab is the vocabulary size, got {vocab!r}")
        check_k(idx.shape[2], vocab)
        if not isinstance(temperature, numbers.Real) or not float(temperature) > 0.0:
            raise ValueError(f"TeacherTopK: temperature > 0, got {temperature!r}")
        self.idx, self.logp, self.rest = idx, logp, rest
        self.temperature, self.vocab = float(temperature), int(vocab)

    @property
    def k(self):
        return int(self.idx.shape[2])

    @property
    def shape(self):
        """(B, Td): the label positions the targets cover."""
        return tuple(self.idx.shape[:2])

    def to(self, device):
        return TeacherTopK(self.idx.to(device), self.logp.to(device), self.rest.to(device), self.temperature, self.vocab)

    def as_dict(self):
        return {"idx": self.idx, "logp": self.logp, "rest": self.rest, "temperature": self.temperature, "vocab": self.vocab,
                "k": self.k}

    @classmethod
    def from_dict(cls, d):
        t = cls(d["idx"], d["logp"], d["rest"], d["temperature"], d["vocab"])
        if "k" in d and int(d["k"]) != t.k:
            raise ValueError(f"TeacherTopK.from_dict: k = {d['k']} but the tensors hold {t.k} columns per position")
        return t

    def trimmed(self, Te):
        """The first Te positions of every sequence (distill.trim_dead_positions cuts the labels the same way)."""
        if Te >= self.idx.shape[1]:
            return self
        return TeacherTopK(self.idx[:, :Te], self.logp[:, :Te], self.rest[:, :Te], self.temperature, self.vocab)

    def rows(self, index=None):
        """-> idx [R, k], logp [R, k], rest [R], contiguous: the B * Td positions in (batch, position) order, or the rows `index`
        (int32 / int64 row numbers b * Td + t: engine.LiveRows.idx) lists, in its order -- the trainer's packed rows."""
        k = self.k
        idx, logp, rest = self.idx.reshape(-1, k), self.logp.reshape(-1, k), self.rest.reshape(-1)
        if index is not None:
            index = index.to(torch.int64)
            idx, logp, rest = idx.index_select(0, index), logp.index_select(0, index), rest.index_select(0, index)
        return idx.contiguous(), logp.contiguous(), rest.contiguous()

    def check(self, labels_shape, temperature, vocab):
        """ValueError unless these targets fit a step over labels of `labels_shape` at `temperature` and vocabulary `vocab`."""
        if self.temperature != float(temperature):
            raise ValueError(f"teacher_topk was made at temperature {self.temperature:g}, this call uses {float(temperature):g}: the "
                             "targets are bound to the temperature they were made with")
        if self.vocab != int(vocab):
            raise ValueError(f"teacher_topk was made over a vocabulary of {self.vocab}, the student's is {int(vocab)}")
        if self.shape != tuple(labels_shape):
            raise ValueError(f"teacher_topk covers positions {self.shape}, the labels are {tuple(labels_shape)}")
        check_k(self.k, vocab)


# ---- torch statements of the kernels ---------------------------------------------------------------------------------------------
def logits_topk_torch(logits, V, temperature, k):
    """What `dw_logits_topk` computes, in fp32: logits [rows, >= V] (bf16 values in any float dtype) -> idx int32 [rows, k],
    logp f32 [rows, k], rest f32 [rows].  A stable descending sort keeps equal values in column order: the lower column wins."""
    z = logits[:, :V].to(torch.float32)
    inv_t = torch.tensor(1.0 / float(temperature), dtype=torch.float32, device=z.device)
    order = torch.sort(z + 0.0, dim=-1, descending=True, stable=True).indices[:, :k]
    m = z.max(-1, keepdim=True).values
    e = torch.exp((z - m) * inv_t)                  # one exponential per column: Z over all of them, the tail over the others
    Z = e.sum(-1, keepdim=True)
    logp = (z.gather(1, order) - m) * inv_t - torch.log(Z)
    tail = e.scatter(1, order, 0.0)
    return order.to(torch.int32), logp, tail.sum(-1) / Z[:, 0]


def distill_loss_topk_torch(s_logits, idx, logp, rest, labels, V, temperature, ce_weight, kl_weight, grad_scale, want_grad,
                            grad_out=None, weights_dev=None, return_rows=False):
    """What `dw_distill_loss_topk` computes, in fp32 and with its formulas (csrc/topk_distill.hip header), gradient included: no
    autograd.  Rows whose label excludes them from both sums are not looked at: their idx / logp / rest may hold anything."""
    f32 = torch.float32
    zs = s_logits[:, :V].to(f32)
    rows = zs.shape[0]
    T = float(temperature)
    inv_t = torch.tensor(1.0 / T, dtype=f32, device=zs.device)
    if weights_dev is not None:
        ce_weight, kl_weight = weights_dev[0].detach(), weights_dev[1].detach()
    counted = labels != -100
    ce_ok = counted & (labels >= 0) & (labels < V)
    kl_ok = labels >= 0
    n_ce, n_kl = counted.sum().to(f32), kl_ok.sum().to(f32)
    ms = zs.max(-1, keepdim=True).values
    e1, eT = torch.exp(zs - ms), torch.exp((zs - ms) * inv_t)
    zs1, zsT = e1.sum(-1), eT.sum(-1)
    logZ = torch.log(zsT)
    # the targets of the rows that count; everything else is replaced before it is used
    valid = kl_ok[:, None] & (idx >= 0) & (idx < V)
    col = torch.where(valid, idx, torch.zeros_like(idx)).to(torch.int64)
    lp = torch.where(valid, logp, torch.zeros_like(logp))
    p = torch.where(valid, torch.exp(lp), torch.zeros_like(lp))
    r = torch.where(kl_ok, rest, torch.zeros_like(rest))
    member = torch.zeros(rows, V, dtype=torch.int32, device=zs.device).scatter_add_(1, col, valid.to(torch.int32)) > 0
    tail = (eT * (~member)).sum(-1).clamp_min(FLT_MIN)          # the non-members' own terms, never "whole minus the members"
    kl_members = (p * (lp - ((zs.gather(1, col) - ms) * inv_t - logZ[:, None]))).sum(-1)
    r_safe = torch.where(r > 0, r, torch.ones_like(r))
    kl_rest = torch.where(r > 0, r * (torch.log(r_safe) - (torch.log(tail) - logZ)), torch.zeros_like(r))
    z_label = zs.gather(1, torch.where(ce_ok, labels, torch.zeros_like(labels))[:, None])[:, 0]
    zero = torch.zeros(rows, dtype=f32, device=zs.device)
    row_ce = torch.where(ce_ok, ms[:, 0] + torch.log(zs1) - z_label, zero)
    row_kl = torch.where(kl_ok, kl_members + kl_rest, zero)
    ce = row_ce.sum() / n_ce                                     # (0 / 0 = NaN for a batch without labels, as the kernel reports it)
    kl = row_kl.sum() / n_kl * (T * T)
    losses = torch.stack([ce, kl, ce_weight * ce + kl_weight * kl, n_ce]).to(f32)
    if want_grad:
        gce = torch.where(ce_ok, grad_scale * ce_weight / n_ce.clamp_min(1.0), zero)
        gkl = torch.where(kl_ok, grad_scale * kl_weight * T / n_kl.clamp_min(1.0), zero)
        i1, iS = 1.0 / zs1, 1.0 / zsT
        ftail = iS - torch.where(r > 0, r / tail, zero)
        onehot = torch.zeros_like(zs).scatter_(1, torch.where(ce_ok, labels, torch.zeros_like(labels))[:, None], ce_ok.to(f32)[:, None])
        p_dense = torch.zeros_like(zs).scatter_add_(1, col, p)
        gk = torch.where(member, eT * iS[:, None] - p_dense, eT * ftail[:, None])
        g = gce[:, None] * (e1 * i1[:, None] - onehot) + gkl[:, None] * gk
        g = torch.where((ce_ok | kl_ok)[:, None], g, torch.zeros_like(g))
        dst = s_logits if grad_out is None else grad_out
        dst.zero_()
        dst[:, :V] = g.to(dst.dtype)
    return (losses, row_ce, row_kl) if return_rows else losses


# ---- through an ops object: its kernels where it has them, the statements above otherwise -----------------------------------------
def logits_topk(ops, logits, V, temperature, k):
    fn = getattr(ops, "logits_topk", None)
    return fn(logits, V, temperature, k) if fn is not None else logits_topk_torch(logits, V, temperature, k)


def distill_loss_topk(ops, s_logits, idx, logp, rest, labels, V, temperature, ce_weight, kl_weight, grad_scale, want_grad, **kw):
    fn = getattr(ops, "distill_loss_topk", None)
    if fn is not None:
        return fn(s_logits, idx, logp, rest, labels, V, temperature, ce_weight, kl_weight, grad_scale, want_grad, **kw)
    return distill_loss_topk_torch(s_logits, idx, logp, rest, labels, V, temperature, ce_weight, kl_weight, grad_scale, want_grad, **kw)


def scatter_targets(idx, logp, rest, B, T, index=None, Te=None):
    """Targets of the computed rows -> zero-filled rectangles idx / logp [B, T, k], rest [B, T].  `index` (LiveRows.idx): the rows
    are the packed live rows of the [B, Te] rectangle; otherwise they are all B * Te rows.  Dead positions stay zero; they are never
    read (their labels are -100)."""
    k = idx.shape[1]
    Te = T if Te is None else Te
    oi = torch.zeros(B, Te, k, dtype=torch.int32, device=idx.device)
    ol = torch.zeros(B, Te, k, dtype=torch.float32, device=idx.device)
    orr = torch.zeros(B, Te, dtype=torch.float32, device=idx.device)
    if index is None:
        oi.view(-1, k).copy_(idx)
        ol.view(-1, k).copy_(logp)
        orr.view(-1).copy_(rest)
    else:
        index = index.to(torch.int64)
        oi.view(-1, k).index_copy_(0, index, idx)
        ol.view(-1, k).index_copy_(0, index, logp)
        orr.view(-1).index_copy_(0, index, rest)
    if Te < T:
        pad = lambda t: torch.cat([t, t.new_zeros((B, T - Te) + tuple(t.shape[2:]))], 1)
        oi, ol, orr = pad(oi), pad(ol), pad(orr)
    return oi, ol, orr
