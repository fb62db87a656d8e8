"""Generated-code guard of the grouped weight-gradient kernel (csrc/gemm_wgrad_group.hip), cross-compiled for gfx950, no GPU: the form of
tests/test_codegen.py for the one kernel this translation unit holds.  160 accumulator + 56 fragment + 17 address registers leave the
K loop two dozen to spare: nothing may be parked in scratch inside it (a scratch reload is a VMEM load whose vmcnt wait also waits
for the operand loads in flight), no access may go through a generic pointer, and the LDS is the two 72 KiB stages."""
import os
import re
import shutil

import pytest

from test_codegen import HIPCC, _asm, _lint


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="needs the ROCm compiler")
def test_grouped_weight_gradient_k_loop_has_no_scratch_and_no_flat_accesses():
    lint = _lint()
    asm = _asm(lint, "gemm_wgrad_group")
    kernels = list(lint.kernels(asm))
    assert len(kernels) == 1 and "wgrad_group_kernel" in kernels[0][0]
    name, body = kernels[0]
    _, whole = lint.census(body)
    assert whole["flat"] == 0
    hot = 0
    for a, b, seg in lint.loops(body):
        n, c = lint.census(seg)
        if c["mfma"] > 80 or n > 700:
            continue
        hot += 1
        assert c["mfma"] == 80 and c["ds"] == 56 and c["vmem"] == 9, (a, b, c)      # a K tile: 4 sub-steps of 20, 28 fragments of two reads, 9 pieces
        assert c["scratch"] == 0 and c["flat"] == 0, (a, b, c)
    assert hot == 1
    tail = asm[asm.index(".amdhsa_kernel " + name):]
    assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", tail).group(1)) == 2 * 72 * 1024
    # whole kernel: one quad of registers parked behind the K loop, at the top of the epilogue, reloaded once per copy of its walk
    assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", tail).group(1)) <= 20
    assert sum(1 for l in body if l.strip().startswith("scratch_")) <= 4
