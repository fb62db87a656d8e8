"""TEST INFRASTRUCTURE: the dropout mask generator of csrc/dropout.hip restated in numpy from its definition
(include/dwamd.h dw_dropout_fwd), the three dropout ops in torch with the kernels' rounding points on top of
oracle.ref_ops.RefOps, and a patch that feeds the same masks to a `transformers` Whisper model.

Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11): ten rounds of
    (c0, c1, c2, c3) <- (hi(M1 * c2) ^ c1 ^ k0,  lo(M1 * c2),  hi(M0 * c0) ^ c3 ^ k1,  lo(M0 * c0))
with the key (k0, k1) advanced by (W0, W1) between rounds.
"""
import contextlib

import numpy as np
import torch

from oracle.ref_ops import RefOps

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
_U32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or scalars) of one shape, key: two -> four uint32 arrays."""
    c = [np.asarray(x, dtype=np.uint64) & _U32 for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]              # 32 x 32 -> 64 bit products (no overflow in uint64)
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _U32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _U32]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [x.astype(np.uint32) for x in c]


def threshold(p):
    return min(2**32 - 1, int(round(float(p) * 2.0**32)))


def mask(seed, step, site, rows, cols, p):
    """bool [rows, cols]: True = kept.  Element e = row * cols + col uses word e & 3 of the block with counter
    (e >> 2, site, step_lo, step_hi) under key = seed."""
    n = rows * cols
    assert n < 2**34 and cols % 8 == 0
    seed, step = int(seed) & (2**64 - 1), int(step) & (2**64 - 1)
    blocks = np.arange((n + 3) // 4, dtype=np.uint64)
    w = philox4x32_10((blocks, site, step & 0xFFFFFFFF, step >> 32), (seed & 0xFFFFFFFF, seed >> 32))
    words = np.stack(w, 1).reshape(-1)[:n]
    return (words >= np.uint32(threshold(p))).reshape(rows, cols)


def pack_mask(m):
    """bool [rows, cols] -> uint8 [rows, cols / 8], bit j of byte b = column 8b + j"""
    return np.packbits(np.asarray(m, dtype=np.uint8), axis=1, bitorder="little")


def unpack_mask(b, cols):
    return np.unpackbits(np.asarray(b, dtype=np.uint8), axis=1, bitorder="little")[:, :cols].astype(bool)


def scale(p):
    """1 / (1 - p) as the float the kernels receive"""
    return float(np.float32(1.0 / (1.0 - p)))


class DropRefOps(RefOps):
    """RefOps + the three dropout ops, with the rounding points of csrc/dropout.hip: the product by 1/(1-p) is an fp32
    multiply, rounded to the low-precision dtype when the operand is low precision; the residual add is in fp32 and
    rounded once by the store."""

    name = "ref-dropout"

    def dropout_state(self, step=0):
        return torch.tensor([int(step)], dtype=torch.int64, device=self.device)

    def dropout_tick(self, state):
        state += 1

    def _scaled(self, x, p):
        t = x.float() * scale(p)
        return t.to(x.dtype).float() if x.dtype != torch.float32 else t

    def dropout_fwd(self, u, p, seed, state, site, residual=None, out=None, out_dtype=None, out_row_pad=0):
        rows, cols = u.shape
        m = mask(seed, int(state.item()), site, rows, cols, p)
        mt = torch.from_numpy(m).to(u.device)
        t = torch.where(mt, self._scaled(u, p), torch.zeros((), device=u.device))
        v = t if residual is None else residual[:rows].float() + t
        dt = out.dtype if out is not None else (u.dtype if out_dtype is None else out_dtype)
        v = v.to(dt)
        if out is not None:
            out.copy_(v)
            v = out
        return v, torch.from_numpy(pack_mask(m)).to(u.device)

    def dropout_bwd(self, dy, mask, p, out=None):       # noqa: A002 -- the ops interface's argument name
        rows, cols = dy.shape
        mt = torch.from_numpy(unpack_mask(mask.cpu().numpy(), cols)).to(dy.device)
        v = torch.where(mt, self._scaled(dy, p), torch.zeros((), device=dy.device)).to(dy.dtype if out is None else out.dtype)
        if out is not None:
            out.copy_(v)
            v = out
        return v


@contextlib.contextmanager
def patched_dropout(seed, step, sites):
    """Inside the block `torch.nn.functional.dropout` multiplies by the restated mask of the next entry of `sites` times
    1/(1-p): one entry per call with p > 0 in training mode, in call order.  Calls with p == 0 or training=False pass
    through.  The tensor is [..., cols]; its leading dimensions flatten to the rows."""
    import torch.nn.functional as F
    orig, todo = F.dropout, list(sites)

    def dropout(x, p=0.5, training=True, inplace=False):
        if p == 0 or not training:
            return x
        assert todo, "more dropout calls than sites"
        site, cols, want_p = todo.pop(0)
        assert x.shape[-1] == cols and abs(want_p - p) < 1e-12, (site, tuple(x.shape), cols, p, want_p)
        m = mask(seed, step, site, x.numel() // cols, cols, p)
        return x * (torch.from_numpy(m).to(x.device).reshape(x.shape).to(x.dtype) * scale(p))

    F.dropout = dropout
    try:
        yield todo
    finally:
        F.dropout = orig
