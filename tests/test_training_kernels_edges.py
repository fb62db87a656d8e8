"""CPU companion of tests/test_training_kernels_edges_gpu.py: the float64 restatements of tests/training_restatement.py against torch's own
float64 LayerNorm / cross-entropy / KL autograd, AdamW and clip_grad_norm_ (1e-12 relative), and the case tables against what the
GPU module promises of them (every width, row count, vocabulary and vector-length class, every kernel instantiation)."""
import pytest
import torch
import torch.nn.functional as F

import training_restatement as tr

TOL = 1e-12


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


# ---- restatements against torch float64 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", tr.LN_DTYPES)
@pytest.mark.parametrize("rows,cols", [(1, 4), (5, 260), (517, 1028), (33, 2048)])
def test_layernorm_restatement_equals_torch_autograd(rows, cols, dtype):
    x, gamma, beta, dy, dres = tr.ln_inputs(rows, cols, dtype)
    eps = tr.f32_as_double(tr.LN_EPS)
    x64 = x.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    want = F.layer_norm(x64, (cols,), g64, b64, eps)
    want.backward(dy.double())
    y, mean, rstd = tr.layernorm_fwd(x, gamma, beta)
    assert rel(y, want.detach()) <= TOL
    assert rel(mean, x.double().mean(-1)) <= TOL and rel(rstd, (x.double().var(-1, unbiased=False) + eps).rsqrt()) <= TOL
    out, dgamma, dbeta, lo, cs = tr.layernorm_bwd(dy, x, mean, rstd, gamma, dres, lowp=True)
    # (the constant rows have x_hat = 0 and a gradient of rsqrt(eps) * (g - mean(g)): 316 times the others, still 1e-12 relative)
    assert rel(out - dres.double(), x64.grad) <= TOL and rel(dgamma, g64.grad) <= TOL and rel(dbeta, b64.grad) <= TOL
    assert lo.dtype == torch.bfloat16 and torch.equal(lo, out.float().to(torch.bfloat16)) and torch.equal(cs, lo.double().sum(0))
    out0, _, _ = tr.layernorm_bwd(dy, x, mean, rstd, gamma, None)
    assert rel(out0, x64.grad) <= TOL


def _torch_loss(s, t, labels, V, T, ce_w, kl_w, grad_scale):
    """F.cross_entropy + the softmax / log_softmax / kl_div / mask lines of RefOps.distill_loss, in float64."""
    zs = s[:, :V].double().requires_grad_(True)
    zt = t[:, :V].double()
    ce = F.cross_entropy(zs, labels, ignore_index=-100)
    teacher = F.softmax(zt / T, dim=-1)
    student = F.log_softmax(zs / T, dim=-1)
    div = F.kl_div(student, teacher, reduction="none")
    mask = (labels >= 0).unsqueeze(-1)
    kl = (div * mask).sum() / mask.sum() * T ** 2
    total = ce_w * ce + kl_w * kl
    (g,) = torch.autograd.grad(total * grad_scale, zs)
    return ce.detach(), kl.detach(), total.detach(), g, F.cross_entropy(zs, labels, ignore_index=-100, reduction="none").detach(), \
        (div * mask).sum(-1).detach()


@pytest.mark.parametrize("case", [c for c in tr.loss_cases() if c[0] <= 4097 and c[3] != "ignored"], ids=str)
def test_loss_restatement_equals_torch_autograd(case):
    V, ld, rows, kind, T, (ce_w, kl_w), gs, regime = case
    s, t, labels = tr.loss_inputs(V, ld, rows, regime, kind)
    assert s.shape == (rows, ld) and bool((labels < V).all()) and bool((s[:, V:] == tr.LOSS_PAD).all())
    ce, kl, total, g, rce, rkl = _torch_loss(s, t, labels, V, T, ce_w, kl_w, gs)
    row_ce, row_kl, losses, grad = tr.distill_loss(s, t, labels, V, T, ce_w, kl_w, gs)
    scale = lambda x: x.abs().max().clamp_min(1e-300)
    if regime == "equal":       # exactly zero in float64, on both sides
        assert not bool(row_kl.any()) and losses[1].item() == 0.0 and abs(kl.item()) <= 1e-15
    elif regime == "near":      # KL of 1e-4 from terms of 1e-2 that cancel: what float64 leaves of either side is 1e-16 absolute
        assert abs(losses[1] - kl) <= 1e-14 * T * T and (row_kl - rkl).abs().max() <= 1e-14
    else:
        assert abs(losses[1] - kl) <= TOL * abs(kl) and (row_kl - rkl).abs().max() <= TOL * scale(rkl)
    if regime == "spiked":      # CE of 1e-13: the cancellation in lse - z[label] leaves 1e-15 absolute on either side
        assert (row_ce - rce).abs().max() <= 1e-14 and abs(losses[0] - ce) <= 1e-14
    else:
        assert (row_ce - rce).abs().max() <= TOL * scale(rce) and abs(losses[0] - ce) <= TOL * abs(ce)
        assert abs(losses[2] - total) <= TOL * abs(total) + (1e-14 * T * T if regime in ("near", "equal") else 0.0)
    assert losses[3].item() == float((labels != -100).sum())
    if regime == "equal" and ce_w == 0.0:
        assert not bool(grad.any())
    elif regime != "spiked":
        assert rel(grad, g) <= TOL
    else:                       # (p[label] - 1 cancels to 1e-13 there: absolute, on the scale of the gradient's weights)
        assert (grad - g).abs().max() <= 1e-14 * gs
    assert not bool(grad[labels == -100].any())


def test_loss_restatement_of_an_all_ignored_batch():
    s, t, labels = tr.loss_inputs(9, 16, 3, "gauss", "ignored")
    row_ce, row_kl, losses, grad = tr.distill_loss(s, t, labels, 9, 2.0, 0.8, 1.0, 1.0)
    assert bool(torch.isnan(losses[:3]).all()) and losses[3].item() == 0.0
    assert not bool(grad.any()) and not bool(row_ce.any()) and not bool(row_kl.any())


@pytest.mark.parametrize("branch", tr.ADAMW_BRANCHES, ids=lambda b: b["name"])
@pytest.mark.parametrize("n", [1, 5, 1027])
def test_adamw_restatement_equals_torch_adamw_and_clip_grad_norm(n, branch):
    p, g, m, v = tr.adamw_inputs(n)
    m, v = torch.zeros_like(m), torch.zeros_like(v)         # torch.optim.AdamW starts from zero moments
    h = tr.ADAMW_HYPER
    ss = tr.sumsq(g)
    assert abs(ss - torch.linalg.vector_norm(g.double()) ** 2) <= TOL * ss
    norm = ss.sqrt().item() * abs(branch["grad_mul"])
    max_norm = 0.0 if not branch["clip"] else branch["clip"] * norm
    got = tr.adamw_steps(p, g, m, v, None if branch["clip"] is None else ss, max_norm, branch["grad_mul"], h["lr"], h["betas"], h["eps"],
                         branch["wd"], tr.ADAMW_STEPS)
    w = torch.nn.Parameter(p.double())
    opt = torch.optim.AdamW([w], lr=h["lr"], betas=h["betas"], eps=h["eps"], weight_decay=branch["wd"])
    for _ in range(tr.ADAMW_STEPS):
        w.grad = g.double() * branch["grad_mul"]
        if max_norm > 0 and branch["clip"] is not None:
            total = torch.nn.utils.clip_grad_norm_([w], max_norm)
            assert (total.item() > max_norm) == (branch["clip"] < 1)
        opt.step()
    st = opt.state[w]
    assert rel(got[0], w.detach()) <= TOL and rel(got[1], st["exp_avg"]) <= TOL and rel(got[2], st["exp_avg_sq"]) <= TOL


def test_metric_and_ulp_helpers():
    x = torch.tensor([1.0, 1.5, 255.0, 256.0, -0.75, 0.0], dtype=torch.float64)
    assert tr.bf16_ulp(x).tolist() == [2.0 ** -7, 2.0 ** -7, 1.0, 2.0, 2.0 ** -8, 0.0]
    ref = torch.tensor([[3.0, 4.0], [0.0, 0.0]], dtype=torch.float64)
    off = ref + torch.tensor([[0.0, 0.5], [0.1, 0.0]], dtype=torch.float64)
    rms = (25.0 / 2) ** 0.5
    assert abs(tr.row_err(off, ref, 2) - max(0.5 / 5.0, 0.1 / rms)) < 1e-15


# ---- the case tables hold what the GPU module's headings promise ---------------------------------------------------------------------
def test_layernorm_tables_reach_every_instantiation():
    assert tr.LN_COLS == [4, 8, 252, 256, 260, 512, 516, 768, 772, 1024, 1028, 1276, 1280, 1284, 1540, 1544, 2044, 2048]
    assert tr.LN_ROWS == [1, 3, 5, 517] and tr.LN_DTYPES == [torch.float32, torch.bfloat16]
    fwd = {tr.ln_fwd_kernel(r, c, d) for c in tr.LN_COLS for r in tr.LN_ROWS for d in tr.LN_DTYPES}
    want = {f"ln_fwd_kernel<false,{nv}>" for nv in (2, 3, 5, 8)} | {f"ln_fwd_kernel<true,{nv}>" for nv in (2, 3, 5, 8)}
    want |= {f"ln_fwd_bf16x8_kernel<{nv},true>" for nv in (1, 2, 3, 4)}
    assert fwd == want                                        # <true,.>: the widths with cols % 8 == 4
    assert {tr.ln_fwd_kernel(5, c, torch.bfloat16, sixteen_byte=False) for c, _ in tr.LN_FALLBACK} == \
        {"ln_fwd_bf16x8_kernel<1,false>", "ln_fwd_bf16x8_kernel<3,false>"}
    assert {how for _, how in tr.LN_FALLBACK} == {"pitch+4", "base+8B"}
    # a partially filled last vector (one live lane in the last j), and a full one, in every width class
    for lo, hi in ((4, 512), (516, 768), (772, 1280), (1284, 2048)):
        cls = [c for c in tr.LN_COLS if lo <= c <= hi]
        assert any((c // 4) % 64 == 1 for c in cls) and any((c // 4) % 64 == 0 for c in cls), (lo, hi)
    assert tr.ln_bwd_kernel(5, 1024)[0] == "ln_bwd_kernel<.,5,12>" and tr.ln_bwd_kernel(5, 1028)[0] == "ln_bwd_pf_kernel<.,5,8>"
    bwd = {tr.ln_bwd_kernel(r, c)[0] for c in tr.LN_COLS for r in tr.LN_ROWS}
    assert bwd == {"ln_bwd_kernel<.,2,4>", "ln_bwd_kernel<.,3,4>", "ln_bwd_kernel<.,5,12>", "ln_bwd_kernel<.,8,4>", "ln_bwd_pf_kernel<.,5,8>"}
    # persistent forward: narrow rows, a partial last vector, the threshold from both sides
    assert tr.LN_PERSIST == [(8192, 384), (8192, 1024), (8195, 260), (8191, 1280)]
    names = [tr.ln_fwd_kernel(r, c, torch.float32) for r, c in tr.LN_PERSIST]
    assert names[:3] == ["ln_fwd_persist_kernel<5>"] * 3 and names[3] == "ln_fwd_kernel<false,5>"
    assert all(tr.ln_fwd_kernel(r, c, torch.float32, variant=2) != "ln_fwd_persist_kernel<5>" for r, c in tr.LN_PERSIST)
    # backward: every row loop wraps, by a remainder that leaves some waves one row short
    assert tr.LN_WRAP == [(4101, 384), (4101, 768), (3077, 1024), (1029, 2048), (2053, 1280)]
    for rows, cols in tr.LN_WRAP:
        name, per_pass = tr.ln_bwd_kernel(rows, cols)
        assert per_pass < rows < 2 * per_pass, (rows, cols)
    assert {tr.ln_bwd_kernel(r, c)[0] for r, c in tr.LN_WRAP} == bwd
    assert all(tr.ln_bwd_kernel(r, c)[1] >= 517 for c in tr.LN_COLS for r in tr.LN_ROWS)       # (none of the sweep's cases wraps)
    assert tr.LN_PREFETCH_OFF == [(2053, 1280), (517, 1028)]
    for rows, cols in tr.LN_PREFETCH_OFF:
        assert tr.ln_bwd_kernel(rows, cols)[0] == "ln_bwd_pf_kernel<.,5,8>" and tr.ln_bwd_kernel(rows, cols, variant=1)[0] == "ln_bwd_kernel<.,5,12>"
    assert tr.ln_bwd_kernel(2053, 1280)[1] < 2053 and tr.ln_bwd_kernel(2053, 1280, variant=1)[1] > 2053
    x = tr.ln_inputs(8, 16, torch.float32)[0]
    assert tr.LN_KINDS == ("gauss", "outliers", "constant", "small")
    assert x[1].max() == 300 and x[1].min() == -300 and bool((x[2] == 1.5).all()) and x[3].abs().max() < 1e-2 and x[4].abs().max() > 0.5


def test_loss_table_holds_every_class():
    cases = tr.loss_cases()
    assert len(set(cases)) == len(cases)
    assert tr.LOSS_VLD == [(5, 8), (8, 8), (9, 16), (1000, 1000), (2047, 2048), (2049, 2056), (4097, 4104), (51866, 51872), (51866, 51968)]
    for V, ld in tr.LOSS_VLD:
        mine = [c for c in cases if c[:2] == (V, ld)]
        assert {c[2] for c in mine} == {1, 3, 97} and {c[3] for c in mine} == {"random", "edges", "ignored"}
    assert {c[4] for c in cases} == {1.0, 2.0, 4.0}
    assert {c[5] for c in cases} == {(0.8, 1.0), (1.0, 0.0), (0.0, 1.0)}
    assert {c[6] for c in cases} == {1.0, 0.125, 1024.0}
    assert {c[7] for c in cases} == set(tr.LOSS_REGIMES) == {"gauss", "equal", "near", "spiked"}
    big = [c for c in cases if c[0] == 51866]
    assert {c[7] for c in big if c[2] == 97} == set(tr.LOSS_REGIMES) and {c[4] for c in big} == {1.0, 2.0, 4.0}
    assert max(c[2] for c in cases) == 97
    assert any(c[5] == (0.0, 1.0) and c[7] == "equal" for c in cases)          # the identically zero gradient
    # V < 8, V < 2048, one past a multiple of 2048 (twice), a last vector with 1, 2, 7 and 8 live columns
    vs = [V for V, _ in tr.LOSS_VLD]
    assert min(vs) < 8 and any(V % 2048 == 1 for V in vs) and {V % 8 for V in vs} >= {0, 1, 2, 5, 7}
    # labels 0 and V - 1 are present wherever the table says "edges"
    for V, ld, rows, kind, *_ in cases:
        if kind == "edges":
            lab = tr.loss_inputs(V, ld, rows, "gauss", kind)[2] if V <= 4097 else None
            assert lab is None or (lab[0] == 0 and (rows < 2 or lab[1] == V - 1))
    assert tr.LOSS_WAYS == ["in_place", "grad_out", "weights_dev"]


def test_adamw_table_holds_every_class():
    assert tr.ADAMW_N == [1, 3, 4, 5, 1027, 2048 * 1024 + 1027, 4096 * 1024 + 1027]
    assert sum(n > tr.SUMSQ_GRID_PASS for n in tr.ADAMW_N) == 2 and sum(n > tr.ADAMW_GRID_PASS for n in tr.ADAMW_N) == 1
    assert all(n % 4 for n in tr.ADAMW_N if n > 1027) and any(n < 4 for n in tr.ADAMW_N)
    b = {x["name"]: x for x in tr.ADAMW_BRANCHES}
    assert b["clipping"]["clip"] < 1 < b["below_max_norm"]["clip"] and b["max_norm_0"]["clip"] == 0 and b["sumsq_none"]["clip"] is None
    assert {x["grad_mul"] for x in tr.ADAMW_BRANCHES} == {1.0, 0.5, 1.0 / 1024}
    assert {x["wd"] for x in tr.ADAMW_BRANCHES} == {0.0, 0.01} and {x["shadow"] for x in tr.ADAMW_BRANCHES} == {True, False}
    assert set(tr.ADAMW_BIG_BRANCHES) <= set(b) and tr.ADAMW_STEPS == 3
