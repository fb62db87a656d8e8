"""Kernel outputs inside NaN-patterned buffers (GPU tests): whatever a kernel writes outside its live view changes a guard element,
and intact() compares the pattern bit for bit."""
import torch

from attention_restatement import NAN16, NAN32

DEV = "cuda:0"


def _fill(buf):
    if buf.dtype == torch.bfloat16:
        buf.view(torch.int16).fill_(NAN16)
    else:
        assert buf.dtype == torch.float32
        buf.view(torch.int32).fill_(NAN32)


def _bits(buf):
    return (buf.view(torch.int16), NAN16) if buf.dtype == torch.bfloat16 else (buf.view(torch.int32), NAN32)


class Guarded:
    """A [rows, cols] output (bf16, or fp32 with dtype=torch.float32) inside a larger NaN-patterned buffer: `pad` extra columns per
    row, the live columns starting at column `off`, guard rows behind.  intact(): every element outside the live view still holds the
    pattern, bit for bit."""

    def __init__(self, rows, cols, pad=8, off=0, guard_rows=3, dtype=torch.bfloat16):
        self.buf = torch.empty(rows + guard_rows, cols + pad, dtype=dtype, device=DEV)
        _fill(self.buf)
        self.rows, self.cols, self.off = rows, cols, off
        self.live = self.buf[:rows, off:off + cols]

    def intact(self):
        bits, pattern = _bits(self.buf)
        g = bits.clone()
        g[:self.rows, self.off:self.off + self.cols] = pattern
        return bool((g == pattern).all())

    def untouched(self):
        bits, pattern = _bits(self.buf)
        return bool((bits == pattern).all())


class Guarded32:
    """n live floats with `guard` patterned slots behind them."""

    def __init__(self, n, guard=16, zero=False):
        self.buf = torch.empty(n + guard, dtype=torch.float32, device=DEV)
        self.buf.view(torch.int32).fill_(NAN32)
        self.live = self.buf[:n]
        if zero:
            self.live.zero_()

    def intact(self):
        return bool((self.buf[self.live.numel():].view(torch.int32) == NAN32).all())

    def untouched(self):
        return bool((self.buf.view(torch.int32) == NAN32).all())
