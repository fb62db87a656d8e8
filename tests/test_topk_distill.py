"""Offline distillation from stored top-k teacher targets, on the CPU: the float64 restatement (tests/topk_distill_restatement.py) against
central differences, the dense loss and the bucket bound; the torch statements of distil_whisper_amd/topk_distill.py against float64;
the trainer and the model surface over oracle.ref_ops.RefOps."""
import numpy as np
import pytest
import torch

import topk_distill_restatement as tk
import training_restatement as tr
from distil_whisper_amd import TeacherTopK, topk_distill
from distil_whisper_amd.distill import DistillationTrainer
from oracle.ref_ops import RefOps
from test_engine_cpu import relerr, setup

BF16, F32 = torch.bfloat16, torch.float32
ULP32 = 2.0 ** -23


# ---- the float64 restatement itself ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1.0, 2.0])
@pytest.mark.parametrize("k", [1, 4, 8])
@pytest.mark.parametrize("V", [9, 37])
def test_restatement_gradient_matches_central_differences(V, k, T):
    g = torch.Generator().manual_seed(V + 10 * k)
    s = torch.randn(3, V, generator=g, dtype=torch.float64) * 2.0
    t = (torch.randn(3, V, generator=g) * 2.0).to(BF16)
    labels = torch.tensor([V - 1, -100, 0])
    idx, logp, rest = tk.targets(t, V, T, k)
    _, _, losses, grad = tk.loss(s, idx, logp, rest, labels, V, T, 0.8, 1.3, 1.0)
    h = 1e-6
    num = torch.zeros_like(s)
    for r in range(3):
        for c in range(V):
            sp, sm = s.clone(), s.clone()
            sp[r, c] += h
            sm[r, c] -= h
            num[r, c] = (tk.loss(sp, idx, logp, rest, labels, V, T, 0.8, 1.3, 1.0)[2][2] -
                         tk.loss(sm, idx, logp, rest, labels, V, T, 0.8, 1.3, 1.0)[2][2]) / (2 * h)
    assert (grad - num).abs().max().item() < 1e-8
    assert not bool(grad[1].any())


@pytest.mark.parametrize("T", [1.0, 2.0])
def test_dense_limit(T):
    """Teacher rows whose tail lies 200 T below the k-th value: rest == 0 in fp32, loss and gradient are the dense ones."""
    V, k, rows = 37, 4, 5
    g = torch.Generator().manual_seed(3)
    t = torch.full((rows, V), -260.0 * T)
    cols = torch.stack([torch.randperm(V, generator=g)[:k] for _ in range(rows)])
    t.scatter_(1, cols, torch.randn(rows, k, generator=g) * 2.0)
    t = t.to(BF16)
    s = (torch.randn(rows, V, generator=g) * 2.0).to(BF16)
    labels = torch.tensor([1, -100, 5, V - 1, 0])
    idx, logp, rest = tk.targets(t, V, T, k)
    assert not np.float32(rest).any()
    _, lp32, r32 = topk_distill.logits_topk_torch(t, V, T, k)
    assert not bool(r32.any())
    ce, kl, losses, grad = tk.loss(s, idx, logp, np.zeros_like(rest), labels, V, T, 0.8, 1.0, 1.0)
    dce, dkl, dlosses, dgrad = tk.dense_loss(s, t, labels, V, T, 0.8, 1.0, 1.0)
    assert (ce - dce).abs().max().item() < 1e-13 and (kl - dkl).abs().max().item() < 1e-12
    assert (losses - dlosses).abs().max().item() < 1e-12 and (grad - dgrad).abs().max().item() < 1e-14


@pytest.mark.parametrize("regime", ["gauss", "spiked"])
def test_bucket_bound_and_monotone_in_k(regime):
    V, rows, T = 1030, 7, 2.0
    s, t, labels = tr.loss_inputs(V, V + 2, rows, regime, "random")
    dense = tk.dense_loss(s, t, labels, V, T, 0.8, 1.0, 1.0)[1]
    prev = None
    for k in (1, 2, 8, 32, 64):
        idx, logp, rest = tk.targets(t, V, T, k)
        row_kl = tk.loss(s, idx, logp, rest, labels, V, T, 0.8, 1.0, 1.0)[1]
        assert bool((row_kl <= dense + 1e-12).all()), k
        assert prev is None or bool((row_kl >= prev - 1e-12).all()), k
        prev = row_kl


# ---- the torch statements ----------------------------------------------------------------------------------------------------------
def check_targets(got, want, V, T):
    """idx exact; logp / rest within fp32 rounding of float64: a few ulps of the magnitudes the terms are differences of."""
    idx, logp, rest = (x.cpu() for x in got)
    widx, wlogp, wrest = want
    assert idx.dtype == torch.int32 and np.array_equal(idx.numpy().astype(np.int64), widx)
    scale = np.abs(wlogp).max() + 1.0
    assert np.abs(logp.double().numpy() - wlogp).max() <= 8 * ULP32 * scale
    assert np.abs(rest.double().numpy() - wrest).max() <= 8 * ULP32 * max(wrest.max(), 1e-30) + 1e-37


@pytest.mark.parametrize("T", [1.0, 2.0])
@pytest.mark.parametrize("V,k", [(9, 1), (9, 8), (37, 4), (1030, 8), (1030, 64)])
def test_selection_statement_with_planted_ties(V, k, T):
    z = tk.tie_rows(V, k)
    check_targets(topk_distill.logits_topk_torch(z, V, T, k), tk.targets(z, V, T, k), V, T)
    padded = torch.cat([z, torch.full((z.shape[0], 3), 3.0e4, dtype=BF16)], 1)
    a, b = topk_distill.logits_topk_torch(padded, V, T, k), topk_distill.logits_topk_torch(z, V, T, k)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def poison(idx, logp, rest, labels, V):
    """Garbage in the rows the label excludes: out-of-range indices, NaN, infinities."""
    idx, logp, rest = idx.clone(), logp.clone(), rest.clone()
    dead = labels < 0
    idx[dead] = V + 12345
    idx[dead, ::2] = -2 ** 31
    logp[dead] = float("nan")
    rest[dead] = float("inf")
    return idx, logp, rest


LOSS_STATEMENT_CASES = [(5, 1, "random", 1.0, (0.8, 1.0), "gauss", 2), (5, 3, "ignored", 2.0, (0.8, 1.0), "gauss", 4),
                        (1030, 3, "edges", 2.0, (0.0, 1.0), "spiked", 8), (1030, 97, "random", 1.0, (1.0, 0.0), "near", 32),
                        (2049, 97, "edges", 2.0, (0.8, 1.0), "gauss", 64), (2049, 3, "random", 1.0, (0.8, 1.0), "spiked", 8),
                        (2049, 1, "edges", 2.0, (0.8, 1.0), "near", 32)]


@pytest.mark.parametrize("V,rows,kind,T,w,regime,k", LOSS_STATEMENT_CASES)
def test_loss_statement_against_float64(V, rows, kind, T, w, regime, k):
    ld = V + (-V) % 8
    s, t, labels = tr.loss_inputs(V, ld, rows, regime, kind)
    if rows > 4:
        labels[2] = -1                              # (a negative label other than -100: counted for the CE mean, looked at by neither term)
    idx, logp, rest = topk_distill.logits_topk_torch(t, V, T, k)
    want = tk.loss(s, idx, logp, rest, labels, V, T, w[0], w[1], 1.0)
    g0 = s.clone()
    losses, row_ce, row_kl = topk_distill.distill_loss_topk_torch(g0, idx, logp, rest, labels, V, T, w[0], w[1], 1.0, True, return_rows=True)
    # garbage in the ignored rows, grad_out, weights_dev, no gradient: the same bits
    g1, s1 = torch.full_like(s, 7.0), s.clone()
    pi, pl, pr = poison(idx, logp, rest, labels, V)
    l1, ce1, kl1 = topk_distill.distill_loss_topk_torch(s1, pi, pl, pr, labels, V, T, 123.0, 456.0, 1.0, True, grad_out=g1,
                                                        weights_dev=torch.tensor(w), return_rows=True)
    l2 = topk_distill.distill_loss_topk_torch(s.clone(), pi, pl, pr, labels, V, T, w[0], w[1], 1.0, False)
    bits = lambda x: x.view(torch.int32 if x.dtype == F32 else torch.int16)
    assert torch.equal(s1, s)
    for a, b in ((l1, losses), (ce1, row_ce), (kl1, row_kl), (g1, g0), (l2, losses)):
        assert torch.equal(bits(a), bits(b))
    assert not bool(g0[:, V:].any())
    n_valid = int((labels != -100).sum())
    assert losses[3].item() == n_valid
    if n_valid == 0:
        assert bool(torch.isnan(losses[:3]).all()) and not bool(g0.any()) and not bool(row_ce.any()) and not bool(row_kl.any())
        return
    row_ce64, row_kl64, losses64, grad64 = want
    assert tr.row_err(losses[:3], losses64[:3], 3) < 2e-6
    scale = (torch.logsumexp(s[:, :V].double(), 1).abs().max().item() + s.double()[:, :V].abs().max().item()) * max(1.0, 1.0 / T)
    assert (row_ce.double() - row_ce64).abs().max().item() <= 8 * ULP32 * scale
    assert (row_kl.double() - row_kl64).abs().max().item() <= 16 * ULP32 * scale
    assert tr.row_err(g0[:, :V], grad64, V) < 4e-3            # (bf16 rounding of the gradient: 2^-9 per element)
    res = ((g0[:, :V].double() - tr.to_bf16(grad64).double()).abs() - tr.bf16_ulp(grad64)).clamp_min(0.0)
    assert res.max().item() <= 1e-9 * grad64.abs().max().item()
    assert not bool(g0[:, :V][grad64 == 0].any())


@pytest.mark.parametrize("shift,T", [(120.0, 1.0), (200.0, 2.0)])
def test_loss_statement_rows_far_below_zero(shift, T):
    """Student rows whose largest logit lies below -88 (exp(0 - max) overflows fp32): softmax is shift invariant, the row stays finite
    and is judged like the others."""
    V, rows, k = 1030, 3, 8
    s, t, labels = tr.loss_inputs(V, V + 2, rows, "gauss", "random")
    s[:, :V] = (s[:, :V].float() - shift).to(BF16)
    assert s[:, :V].float().max().item() < -88.0 * T
    idx, logp, rest = topk_distill.logits_topk_torch(t, V, T, k)
    row_ce64, row_kl64, losses64, grad64 = tk.loss(s, idx, logp, rest, labels, V, T, 0.8, 1.0, 1.0)
    g = s.clone()
    losses, row_ce, row_kl = topk_distill.distill_loss_topk_torch(g, idx, logp, rest, labels, V, T, 0.8, 1.0, 1.0, True, return_rows=True)
    assert bool(torch.isfinite(losses).all()) and bool(torch.isfinite(g.float()).all()) and not bool(g[:, V:].any())
    assert tr.row_err(losses[:3], losses64[:3], 3) < 2e-6
    assert (row_ce.double() - row_ce64).abs().max().item() <= 8 * ULP32 * (shift + 20.0)
    assert (row_kl.double() - row_kl64).abs().max().item() <= 16 * ULP32 * (shift + 20.0) / T
    assert tr.row_err(g[:, :V], grad64, V) < 4e-3


# ---- the container -----------------------------------------------------------------------------------------------------------------
def test_teacher_topk_container():
    idx = torch.zeros(2, 5, 4, dtype=torch.int32)
    logp, rest = torch.zeros(2, 5, 4), torch.zeros(2, 5)
    t = TeacherTopK(idx, logp, rest, 2.0, 100)
    assert (t.k, t.vocab, t.temperature, t.shape) == (4, 100, 2.0, (2, 5))
    d = t.as_dict()
    assert set(d) == {"idx", "logp", "rest", "temperature", "vocab", "k"}
    u = TeacherTopK.from_dict(d).to("cpu")
    assert torch.equal(u.idx, idx) and u.temperature == 2.0
    r = t.rows(torch.tensor([7, 2], dtype=torch.int32))
    assert r[0].shape == (2, 4) and r[2].shape == (2,) and t.rows()[0].shape == (10, 4)
    for bad in (lambda: TeacherTopK(idx.long(), logp, rest, 2.0, 100), lambda: TeacherTopK(idx, logp.double(), rest, 2.0, 100),
                lambda: TeacherTopK(idx, logp, rest[:, :4], 2.0, 100), lambda: TeacherTopK(idx, logp, rest, 0.0, 100),
                lambda: TeacherTopK(idx, logp, rest, 2.0, 4), lambda: TeacherTopK(idx[:, :, :0], logp[:, :, :0], rest, 2.0, 100),
                lambda: TeacherTopK(torch.zeros(2, 5, 65, dtype=torch.int32), torch.zeros(2, 5, 65), rest, 2.0, 100),
                lambda: TeacherTopK.from_dict(dict(d, k=5))):
        with pytest.raises(ValueError):
            bad()


# ---- the trainer over RefOps -------------------------------------------------------------------------------------------------------
class Spy:
    """Counts the calls of an engine's encode / decode."""

    def __init__(self, eng):
        self.n = {"encode": 0, "decode": 0}
        for name in self.n:
            fn = getattr(eng, name)

            def wrapped(*a, _fn=fn, _name=name, **k):
                self.n[_name] += 1
                return _fn(*a, **k)
            setattr(eng, name, wrapped)


def make(shared=False, lowp=torch.float32, seed=3, **kw):
    cfg_t, cfg_s, t_sd, s_sd, batch = setup(seed=seed)
    tr_ = DistillationTrainer(RefOps("cpu", lowp=lowp), s_sd, cfg_s, t_sd, cfg_t, freeze_encoder=shared, share_encoder=shared, **kw)
    return tr_, (cfg_t, cfg_s, t_sd, s_sd), (batch["input_features"], batch["decoder_input_ids"], batch["labels"])


@pytest.mark.parametrize("shared", [False, True])
def test_trainer_step_with_targets_runs_no_teacher(shared):
    a, _, (f, d, l) = make(shared)
    b, _, _ = make(shared)
    dense = a.forward_backward(f, d, l)
    tt = b.teacher_targets(f, d, l, k=8)
    assert tt.temperature == b.temperature and tt.shape == tuple(l.shape) and tt.k == 8
    spy = Spy(b.teacher)
    losses = b.forward_backward(f, d, l, teacher_topk=tt)
    assert spy.n == {"encode": 0, "decode": 0}
    assert abs(losses[0].item() - dense[0].item()) <= 1e-6 * abs(dense[0].item())
    assert losses[1].item() <= dense[1].item() * (1 + 1e-6) and losses[1].item() > 0
    assert losses[3].item() == dense[3].item()
    e = b.eval_step(f, d, l, teacher_topk=TeacherTopK(tt.idx, tt.logp, tt.rest, 1.0, tt.vocab))
    assert spy.n == {"encode": 0, "decode": 0} and bool(torch.isfinite(e).all())


def test_trainer_peaked_teacher_gives_the_dense_gradient():
    """A teacher whose logits are peaked (scaled up until the mass outside the top 8 is below fp32's range): the step with targets
    has the dense step's gradient, within the step tolerance of tests/test_engine_cpu.py (2e-4 per tensor)."""
    a, (cfg_t, cfg_s, t_sd, s_sd), (f, d, l) = make()
    t_sd = dict(t_sd)
    t_sd["model.decoder.embed_tokens.weight"] = t_sd["model.decoder.embed_tokens.weight"] * 4000.0
    ops = RefOps("cpu", lowp=torch.float32)
    a = DistillationTrainer(ops, s_sd, cfg_s, t_sd, cfg_t)
    b = DistillationTrainer(ops, s_sd, cfg_s, t_sd, cfg_t)
    dense = a.forward_backward(f, d, l)
    tt = b.teacher_targets(f, d, l, k=8)
    assert tt.rest.max().item() < 1e-30
    losses = b.forward_backward(f, d, l, teacher_topk=tt)
    assert relerr(losses[:3], dense[:3]) < 2e-5
    sa, sb = a.student_store, b.student_store
    for name in sa.real_names():
        if sa.is_trainable(name):
            assert relerr(sb.g[name], sa.g[name]) < 2e-4, name


def test_trainer_trimmed_and_packed_equal_untrimmed():
    a, _, (f, d, l) = make()
    l = l.clone()
    l[0, 20:] = -100
    l[1, 9:] = -100
    tt = a.teacher_targets(f, d, l, k=8)
    full = a.forward_backward(f, d, l, teacher_topk=tt)
    G = a.student_store.G.clone()
    for vl in (20, [20, 9]):
        b, _, _ = make()
        got = b.forward_backward(f, d, l, teacher_topk=tt, valid_len=vl)
        assert relerr(got[:3], full[:3]) < 1e-5 and relerr(b.student_store.G, G) < 1e-4, vl
        t2 = b.teacher_targets(f, d, l, k=8, valid_len=vl)        # made over the live rows only: the same where a label is
        live = l >= 0
        assert torch.equal(t2.idx[live], tt.idx[live]) and relerr(t2.logp[live], tt.logp[live]) < 1e-5
        assert not bool(t2.idx[0, 20:].any()) and not bool(t2.rest[1, 20:].any())


def test_trainer_accumulation_and_teacherless():
    a, (cfg_t, cfg_s, t_sd, s_sd), (f, d, l) = make()
    tt = a.teacher_targets(f, d, l, k=8)
    halves = [TeacherTopK(tt.idx[i:i + 1], tt.logp[i:i + 1], tt.rest[i:i + 1], tt.temperature, tt.vocab) for i in (0, 1)]
    a.train_step_accumulated([(f[:1], d[:1], l[:1], halves[0]), (f[1:], d[1:], l[1:], halves[1])])
    # against the two micro-batches stepped one by one: the mean of their gradients through one optimizer step, as
    # tests/test_engine_cpu.py holds the dense accumulation (and with its tolerance)
    m0, m1, ref = (DistillationTrainer(RefOps("cpu", lowp=torch.float32), s_sd, cfg_s, t_sd, cfg_t) for _ in range(3))
    m0.forward_backward(f[:1], d[:1], l[:1], teacher_topk=halves[0])
    m1.forward_backward(f[1:], d[1:], l[1:], teacher_topk=halves[1])
    ref.student_store.G.copy_(0.5 * (m0.student_store.G + m1.student_store.G))
    ref.optimizer_step()
    assert relerr(a.student_store.P, ref.student_store.P) < 1e-6
    # teacher-less: no teacher store, no teacher engine; the same numbers; the state dict round trip
    ops = RefOps("cpu", lowp=torch.float32)
    b = DistillationTrainer(ops, s_sd, cfg_s, None, None)
    assert b.teacher is None and b.teacher_store is None
    b.train_step_accumulated([(f[:1], d[:1], l[:1], 37, halves[0]), (f[1:], d[1:], l[1:], halves[1], 37)])
    assert relerr(b.student_store.P, a.student_store.P) < 1e-6
    c = DistillationTrainer(ops, s_sd, cfg_s, None, None)
    c.load_state_dict(b.state_dict())
    assert torch.equal(c.student_store.P, b.student_store.P) and c.step_count == b.step_count == 1
    lb, lc = b.train_step(f, d, l, teacher_topk=tt), c.train_step(f, d, l, teacher_topk=tt)
    assert torch.equal(lb, lc) and torch.equal(c.student_store.P, b.student_store.P)
    assert bool(torch.isfinite(c.eval_step(f, d, l, teacher_topk=TeacherTopK(tt.idx, tt.logp, tt.rest, 1.0, tt.vocab))).all())


class NoOps:
    """An ops object on which every call fails: the argument rules are checked before any of them runs."""

    lowp = torch.float32

    def __getattr__(self, name):
        raise AssertionError(f"ops.{name} reached")


def test_trainer_argument_rules_before_any_op():
    a, (cfg_t, cfg_s, t_sd, s_sd), (f, d, l) = make()
    tt = a.teacher_targets(f, d, l, k=8)
    less = DistillationTrainer(RefOps("cpu", lowp=torch.float32), s_sd, cfg_s, None, None)
    aug = dict(mask_time_prob=0.05, mask_time_length=10, mask_time_min_masks=2, mask_feature_prob=0.0, mask_feature_length=10,
               mask_feature_min_masks=0)
    with_aug = DistillationTrainer(RefOps("cpu", lowp=torch.float32), s_sd, cfg_s, t_sd, cfg_t, spec_augment=aug)
    clean_aug = DistillationTrainer(RefOps("cpu", lowp=torch.float32), s_sd, cfg_s, t_sd, cfg_t, spec_augment=aug, augment_teacher=False)
    for t_ in (a, less, with_aug, clean_aug):
        t_.ops = t_.student.ops = NoOps()
    re = lambda **kw: TeacherTopK(kw.get("idx", tt.idx), kw.get("logp", tt.logp), kw.get("rest", tt.rest), kw.get("T", tt.temperature),
                                  kw.get("vocab", tt.vocab))
    bad = [lambda: a.forward_backward(f, d, l, teacher_topk=re(T=1.0)),
           lambda: a.train_step(f, d, l, teacher_topk=re(T=3.0)),
           lambda: a.eval_step(f, d, l, teacher_topk=tt),                                 # eval uses temperature 1.0
           lambda: a.forward_backward(f, d, l, teacher_topk=re(vocab=tt.vocab + 1)),
           lambda: a.forward_backward(f, d, l[:, :-1], teacher_topk=tt),
           lambda: a.forward_backward(f[:1], d[:1], l[:1], teacher_topk=tt),
           lambda: a.forward_backward(f, d, l, teacher_topk=tt.as_dict()),
           lambda: a.forward_backward(f, d, l, teacher_topk=tt.to("meta")),                # targets on another device than the labels
           lambda: a.eval_step(f, d, l, teacher_topk=re(T=1.0).to("meta")),
           lambda: a.train_step_accumulated([(f, d, l, tt, tt)]),
           lambda: a.teacher_targets(f, d, l, k=0), lambda: a.teacher_targets(f, d, l, k=65),
           lambda: less.forward_backward(f, d, l), lambda: less.train_step(f, d, l), lambda: less.eval_step(f, d, l),
           lambda: less.train_step_accumulated([(f, d, l)]), lambda: less.train_step_graphed(f, d, l),
           lambda: less.teacher_targets(f, d, l),
           lambda: with_aug.forward_backward(f, d, l, teacher_topk=tt)]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(NotImplementedError):
        a.train_step_graphed(f, d, l, teacher_topk=tt)
    with pytest.raises(ValueError):
        DistillationTrainer(RefOps("cpu"), s_sd, cfg_s, None, cfg_t)
    with pytest.raises(AssertionError, match="reached"):       # augment_teacher=False passes the rules and runs
        clean_aug.forward_backward(f, d, l, teacher_topk=tt)


# ---- the model surface -------------------------------------------------------------------------------------------------------------
def test_model_teacher_topk_equals_topk_of_its_own_logits():
    from distil_whisper_amd import WhisperForConditionalGeneration
    from distil_whisper_amd.distill import shift_tokens_right
    cfg_t, cfg_s, t_sd, s_sd, batch = setup(seed=6)
    ops = RefOps("cpu", lowp=torch.float32)
    model = WhisperForConditionalGeneration(cfg_t, ops=ops, state_dict=t_sd)
    f, l = batch["input_features"], batch["labels"].clone()
    l[0, 11:] = -100
    l[1, 30:] = -100
    tt = model.teacher_topk(f, labels=l, k=4, temperature=2.0)
    ids = shift_tokens_right(l, model.dims.pad_token_id, model.dims.decoder_start_token_id)
    enc, _ = model.engine.encode(f.float().contiguous(), save=False)
    logits, _ = model.engine.decode(ids.contiguous(), enc, save=False)
    B, T = l.shape
    idx, logp, rest = topk_distill.logits_topk(ops, logits[:B * T], model.dims.vocab, 2.0, 4)
    assert torch.equal(tt.idx.view(-1, 4), idx) and torch.equal(tt.logp.view(-1, 4), logp) and torch.equal(tt.rest.view(-1), rest)
    assert (tt.k, tt.temperature, tt.vocab, tt.shape) == (4, 2.0, model.dims.vocab, (B, T))
    live = l >= 0
    for vl in (30, [11, 30]):
        t2 = model.teacher_topk(f, decoder_input_ids=ids, k=4, temperature=2.0, valid_len=vl)
        assert torch.equal(t2.idx[live], tt.idx[live]) and relerr(t2.logp[live], tt.logp[live]) < 1e-5
        assert not bool(t2.idx[:, 30:].any()) and (isinstance(vl, int) or not bool(t2.logp[0, 11:].any()))
    t3 = model.teacher_topk(encoder_outputs=enc[:B * model.dims.max_src].view(B, model.dims.max_src, -1), labels=l, k=4)
    assert torch.equal(t3.idx, tt.idx)
    for bad in (dict(k=0), dict(k=65), dict(temperature=0.0)):
        with pytest.raises(ValueError):
            model.teacher_topk(f, labels=l, **bad)
    with pytest.raises(ValueError):
        model.teacher_topk(f)
