"""SpecAugment (`apply_spec_augment`) without a GPU: the numpy restatement of the draws (tests/spec_augment_restatement.py)
against `transformers`' own `_compute_mask_indices` fed the same draws, the package's torch statement against the restatement,
the statistics of the subset draw, the drop-in module on the torch oracle against `transformers` fed the same masks, the config
fields and the trainer's bookkeeping."""
import numpy as np
import pytest
import torch

import dropout_restatement as dr
import spec_augment_restatement as sr
from distil_whisper_amd import spec_augment as sa
from distil_whisper_amd.distill import DistillationTrainer
from distil_whisper_amd.modeling import WhisperConfig, WhisperForConditionalGeneration
from oracle import whisper_oracle as wo
from oracle.ref_ops import RefOps

SEED = 11
B = 5
CASES = [("time",) + c for c in sr.TIME_CASES] + [("feature",) + c for c in sr.FEATURE_CASES]


def _case(axis, axis_len):
    site = sr.SITE_TIME if axis == "time" else sr.SITE_FEATURE
    lengths = sr.time_lengths(axis_len) if axis == "time" else None
    return site, lengths


# ---- 1. the reference's own function fed this path's draws ------------------------------------------------------------------
def reference_mask(eps, rows, B, axis_len, lengths, prob, mask_length, min_masks):
    """`transformers`' `_compute_mask_indices` with numpy's two draws replaced by the given epsilon and row starts: the span
    counts, the dummy padding and the clamp are the reference's own code."""
    from transformers.models.whisper.modeling_whisper import _compute_mask_indices
    todo = list(rows or [])
    rand, choice = np.random.rand, np.random.choice

    def fake_rand(*shape):
        assert shape == (1,)
        return np.array([eps])

    def fake_choice(a, size=None, replace=True, p=None):
        st = todo.pop(0)
        assert replace is False and size == len(st), (size, st)            # the reference computed the same span count
        assert all(0 <= s < len(a) for s in st) and len(set(st)) == len(st)
        return np.array(st, dtype=np.int64)

    am = None
    if lengths is not None:
        am = (torch.arange(axis_len)[None, :] < torch.tensor(lengths)[:, None]).long()
    np.random.rand, np.random.choice = fake_rand, fake_choice
    try:
        m = _compute_mask_indices((B, axis_len), mask_prob=prob, mask_length=mask_length, attention_mask=am, min_masks=min_masks)
    finally:
        np.random.rand, np.random.choice = rand, choice
    assert not todo
    return m


@pytest.mark.parametrize("step", sr.STEPS)
@pytest.mark.parametrize("axis,axis_len,mask_length,prob,min_masks", CASES)
def test_restatement_and_torch_statement_equal_the_reference_function(axis, axis_len, mask_length, prob, min_masks, step):
    site, lengths = _case(axis, axis_len)
    eps, rows = sr.axis_draws(SEED, step, site, B, axis_len, lengths, prob, mask_length, min_masks)
    want = reference_mask(eps, rows, B, axis_len, lengths, prob, mask_length, min_masks)
    got = sr.axis_mask(SEED, step, site, B, axis_len, lengths, prob, mask_length, min_masks)
    assert got.dtype == bool and np.array_equal(got, want)
    if prob == 1e-6:
        assert rows is None and not got.any()                    # max_n == 0: nothing is masked
    elif lengths is not None and mask_length == 10:
        assert rows[3] == [] and rows[4] == [] and len(rows[2]) <= 1        # ten frames hold one span of ten at the most
        assert len(rows[2]) == 1 or (min_masks == 0 and prob < 1.0)
        only_last = np.zeros(axis_len, dtype=bool)
        only_last[-1] = True
        assert np.array_equal(got[3], only_last) and np.array_equal(got[4], only_last)          # the zero-span quirk
    # the package's torch statement draws the same
    mine = sa.axis_mask(SEED, step, site, B, axis_len, lengths, prob, mask_length, min_masks)
    assert np.array_equal(mine.numpy(), got)


def test_statement_of_both_axes_and_application():
    p = sa.normalise(dict(mask_time_prob=0.5, mask_time_length=7, mask_feature_prob=0.3, mask_feature_length=3,
                          mask_feature_min_masks=1))
    x = torch.randn(B, 80, 202, generator=torch.Generator().manual_seed(0))
    lengths = torch.tensor(sr.time_lengths(202), dtype=torch.int32)
    state = torch.tensor([2**32 + 1])
    out, tm, fm = sa.spec_augment_torch(x, SEED, state, p, lengths=lengths, out=torch.empty_like(x), want_masks=True)
    wt, wf = sr.masks(SEED, 2**32 + 1, B, 80, 202, lengths.tolist(), p)
    assert np.array_equal(tm.numpy().astype(bool), wt) and np.array_equal(fm.numpy().astype(bool), wf)
    assert wt.any() and wf.any() and not wt.all() and not wf.all()
    assert np.array_equal(out.numpy().view(np.int32), sr.apply(x.numpy(), wt, wf).view(np.int32))
    y = x.clone()
    same, _, _ = sa.spec_augment_torch(y, SEED, state, p, lengths=lengths)
    assert same is y and torch.equal(y, out)
    assert not np.array_equal(sr.masks(SEED + 1, 1, B, 80, 202, None, p)[0], sr.masks(SEED, 1, B, 80, 202, None, p)[0])
    assert not np.array_equal(sr.masks(SEED, 2, B, 80, 202, None, p)[0], sr.masks(SEED, 1, B, 80, 202, None, p)[0])
    assert not np.array_equal(sr.masks(SEED, 1, B, 80, 202, None, p)[0], sr.masks(SEED, 2**32 + 1, B, 80, 202, None, p)[0])


# ---- 2. the draw ------------------------------------------------------------------------------------------------------------
def test_starts_are_distinct_in_range_and_uniform():
    """Floyd's subset draw at M = 50, n = 5 over 20 000 steps: every start is in [0, 50), the five of a step are distinct, and
    the chi-square statistic of the 100 000 start frequencies against uniform stays below the 99.9 % quantile of chi-square with
    49 degrees of freedom (85.35).  Observed when written (seed 11, row 0, the time site): 31.658."""
    M, n = 50, 5
    counts = np.zeros(M, dtype=np.int64)
    for step in range(20000):
        st = sr.starts(SEED, step, sr.SITE_TIME, 0, n, M)
        assert len(set(st)) == n and min(st) >= 0 and max(st) < M
        counts[st] += 1
    expected = 20000 * n / M
    chi2 = float(((counts - expected) ** 2 / expected).sum())
    print("chi-square", chi2)
    assert chi2 < 85.35
    # rows, sites and the words of one block are separate draws
    assert sr.starts(SEED, 3, sr.SITE_TIME, 0, n, M) != sr.starts(SEED, 3, sr.SITE_TIME, 1, n, M)
    assert sr.starts(SEED, 3, sr.SITE_TIME, 0, n, M) != sr.starts(SEED, 3, sr.SITE_FEATURE, 0, n, M)
    assert sorted(sr.starts(SEED, 3, sr.SITE_TIME, 0, M, M)) == list(range(M))         # n == M: everything


# ---- 3. the drop-in on the torch oracle against transformers ------------------------------------------------------------------
def micro(seed=9, B=2, T=13):
    cfg_t = wo.CONFIGS["micro"]
    t_sd = wo.init_state_dict(cfg_t, seed)
    s_sd, cfg_s = wo.student_from_teacher(t_sd, cfg_t, 2, 1)
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn(B, cfg_s.n_mels, 3000, generator=g) * 0.5
    b = wo.synthetic_batch(cfg_s, B, seed=seed + 1, T=T, with_audio=False)
    return cfg_t, t_sd, cfg_s, s_sd, feats, b["decoder_input_ids"], b["labels"]


def config_kw(cfg, **kw):
    return dict(vocab_size=cfg.vocab, num_mel_bins=cfg.n_mels, d_model=cfg.d_model, encoder_layers=cfg.enc_layers,
                decoder_layers=cfg.dec_layers, encoder_attention_heads=cfg.heads, decoder_attention_heads=cfg.heads,
                encoder_ffn_dim=cfg.ffn, decoder_ffn_dim=cfg.ffn, pad_token_id=cfg.pad_token_id, bos_token_id=0,
                eos_token_id=0, decoder_start_token_id=cfg.decoder_start_token_id, **kw)


AUG = dict(apply_spec_augment=True, mask_time_prob=0.1, mask_time_length=10, mask_time_min_masks=2, mask_feature_prob=0.2,
           mask_feature_length=3, mask_feature_min_masks=1)
AUG_PARAMS = {k: v for k, v in AUG.items() if k != "apply_spec_augment"}


def relerr(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-30)).item()


def test_drop_in_train_mode_matches_transformers_with_the_same_masks():
    import transformers
    _, _, cfg_s, s_sd, feats, ids, labels = micro()
    seed = 5
    model = WhisperForConditionalGeneration(WhisperConfig(**config_kw(cfg_s, **AUG)), ops=RefOps("cpu", lowp=torch.float32),
                                            state_dict=s_sd, dropout_seed=seed)
    model.train()
    hf = transformers.WhisperForConditionalGeneration(transformers.WhisperConfig(**config_kw(cfg_s, **AUG))).float()
    hf.load_state_dict(model.state_dict())
    hf.train()
    lens = [3000, 1777]
    am = (torch.arange(3000)[None, :] < torch.tensor(lens)[:, None]).long()
    tm, fm = sr.masks(seed, 1, 2, cfg_s.n_mels, 3000, lens, AUG_PARAMS)              # the first training forward is step 1
    assert tm.any() and fm.any()
    f_ref, f_mine = feats.clone(), feats.clone()
    with sr.patched_mask_indices([tm, fm]) as left:
        ref = hf(input_features=f_ref, attention_mask=am, decoder_input_ids=ids, labels=labels)
        assert not left
    ref.loss.backward()
    out = model(input_features=f_mine, attention_mask=am, decoder_input_ids=ids, labels=labels)
    assert torch.equal(f_mine, f_ref) and not torch.equal(f_mine, feats)             # the caller's tensor, as the reference leaves it
    assert np.array_equal(f_mine.numpy().view(np.int32), sr.apply(feats.numpy(), tm, fm).view(np.int32))
    print("loss", out.loss.item(), "reference", ref.loss.item())
    assert abs(out.loss.item() - ref.loss.item()) < 2e-5 * abs(ref.loss.item())
    out.loss.backward()
    hf.eval()
    with torch.no_grad():
        plain = hf(input_features=feats.clone(), decoder_input_ids=ids, labels=labels)
    assert relerr(plain.encoder_last_hidden_state, ref.encoder_last_hidden_state) > 1e-2       # the masks matter
    assert relerr(out.encoder_last_hidden_state, ref.encoder_last_hidden_state) < 1e-5
    checked, worst = 0, 0.0
    grads = dict(hf.named_parameters())
    for n, p in model.named_parameters():
        if not p.requires_grad:
            continue
        e = relerr(p.grad, grads[n].grad)
        worst = max(worst, e)
        assert e < 2e-4, (n, e)
        checked += 1
    print("worst gradient relerr", worst)
    assert checked > 30


def test_eval_encoder_outputs_and_switched_off_change_nothing():
    _, _, cfg_s, s_sd, feats, ids, labels = micro()
    ops = RefOps("cpu")
    plain = WhisperForConditionalGeneration(WhisperConfig(**config_kw(cfg_s)), ops=ops, state_dict=s_sd)
    plain.train()
    want = plain(input_features=feats, decoder_input_ids=ids, labels=labels)
    want.loss.backward()

    def same_as_plain(model, **kw):
        x = feats.clone()
        if "encoder_outputs" not in kw:
            kw["input_features"] = x
        got = model(decoder_input_ids=ids, labels=labels, **kw)
        got.loss.backward()
        assert torch.equal(x, feats)
        assert torch.equal(got.loss, want.loss) and torch.equal(torch.as_tensor(got.logits), torch.as_tensor(want.logits))

    on = WhisperForConditionalGeneration(WhisperConfig(**config_kw(cfg_s, **AUG)), ops=ops, state_dict=s_sd)
    assert on.engine.spec == sa.normalise(AUG_PARAMS)
    on.eval()
    same_as_plain(on)
    assert int(on.engine.drop_state.item()) == 0                 # no step was drawn
    on.train()
    same_as_plain(on, encoder_outputs=(want.encoder_last_hidden_state,))
    x = feats.clone()
    masked = on(input_features=x, decoder_input_ids=ids, labels=labels)
    assert not torch.equal(x, feats) and not torch.equal(masked.loss, want.loss)
    off = WhisperForConditionalGeneration(WhisperConfig(**config_kw(cfg_s, **dict(AUG, apply_spec_augment=False))), ops=ops,
                                          state_dict=s_sd)
    off.train()
    same_as_plain(off)
    zero = WhisperForConditionalGeneration(
        WhisperConfig(**config_kw(cfg_s, **dict(AUG, mask_time_prob=0.0, mask_feature_prob=0.0))), ops=ops, state_dict=s_sd)
    zero.train()
    same_as_plain(zero)
    assert off.engine.spec is None and zero.engine.spec is None and zero.engine.drop_state is None
    bf = WhisperForConditionalGeneration(WhisperConfig(**config_kw(cfg_s, **AUG)), ops=ops, state_dict=s_sd, dtype=torch.bfloat16)
    assert bf.engine.spec is None                                # the inference-only model ignores the fields


# ---- 4. config -----------------------------------------------------------------------------------------------------------------
def test_config_defaults_round_trip_and_errors(tmp_path):
    import transformers
    cfg = WhisperConfig()
    ref = transformers.WhisperConfig()
    for k in ("apply_spec_augment", "mask_time_prob", "mask_time_length", "mask_time_min_masks", "mask_feature_prob",
              "mask_feature_length", "mask_feature_min_masks"):
        assert k in WhisperConfig._DEFAULTS and getattr(cfg, k) == getattr(ref, k), k
    assert sa.params_from_config(cfg) is None and sa.params_from_config(ref) is None
    cfg = WhisperConfig(**AUG)
    cfg.save_pretrained(str(tmp_path))
    back = WhisperConfig.from_pretrained(str(tmp_path))
    assert {k: getattr(back, k) for k in AUG} == AUG
    assert sa.params_from_config(back) == sa.normalise(AUG_PARAMS)
    _, _, cfg_s, s_sd, *_ = micro()
    hc = transformers.WhisperConfig(**config_kw(cfg_s, **AUG))                # a transformers config in the package's place
    model = WhisperForConditionalGeneration(hc, ops=RefOps("cpu"), state_dict=s_sd)
    assert model.engine.spec == sa.normalise(AUG_PARAMS)
    model.save_pretrained(str(tmp_path / "m"))
    again = WhisperForConditionalGeneration.from_pretrained(str(tmp_path / "m"), ops=RefOps("cpu"))
    assert again.engine.spec == sa.normalise(AUG_PARAMS)
    # the reference's errors, with its messages
    from transformers.models.whisper.modeling_whisper import _compute_mask_indices
    n_mels = cfg_s.n_mels
    for kw, shape, length in ((dict(mask_time_length=0), (2, 3000), 0), (dict(mask_feature_length=n_mels + 1), (2, n_mels), n_mels + 1)):
        with pytest.raises(ValueError) as want:
            _compute_mask_indices(shape, mask_prob=0.1, mask_length=length)
        with pytest.raises(ValueError) as got:
            WhisperConfig(**config_kw(cfg_s, **dict(AUG, **kw)))
        assert str(got.value) == str(want.value)
        with pytest.raises(ValueError) as got:
            sa.masks(1, 1, 2, n_mels, 3000, None, sa.normalise(dict(AUG_PARAMS, **kw)))
        assert str(got.value) == str(want.value)
    WhisperConfig(**config_kw(cfg_s, **dict(AUG, apply_spec_augment=False, mask_time_length=0)))      # off: not looked at


# ---- 5. trainer -----------------------------------------------------------------------------------------------------------------
class Recording:
    """an ops object that notes the name of every call made through it"""

    def __init__(self, ops):
        self._ops, self.calls = ops, []

    def __getattr__(self, name):
        v = getattr(self._ops, name)
        if not callable(v):
            return v

        def call(*a, **k):
            self.calls.append(name)
            return v(*a, **k)
        return call


def test_trainer_bookkeeping():
    cfg_t, t_sd, cfg_s, s_sd, feats, ids, labels = micro(seed=4)
    with pytest.raises(ValueError, match="augment_teacher=False with share_encoder"):
        DistillationTrainer(RefOps("cpu"), s_sd, cfg_s, t_sd, cfg_t, freeze_encoder=True, share_encoder=True,
                            spec_augment=AUG_PARAMS, augment_teacher=False)
    # everything off: the launch sequence of a trainer built without the arguments
    r0, r1 = Recording(RefOps("cpu")), Recording(RefOps("cpu"))
    a = DistillationTrainer(r0, s_sd, cfg_s, t_sd, cfg_t)
    b = DistillationTrainer(r1, s_sd, cfg_s, t_sd, cfg_t, spec_augment=dict(mask_time_prob=0.0, mask_feature_prob=0.0),
                            augment_teacher=False)
    la, lb = a.train_step(feats, ids, labels), b.train_step(feats, ids, labels)
    assert torch.equal(la, lb) and r0.calls == r1.calls and len(r0.calls) > 50
    assert "dropout" not in b.state_dict() and b.student.drop_state is None
    # on: the caller's tensor is never written; the teacher reads the masked features unless told otherwise
    x = feats.clone()
    c = DistillationTrainer(RefOps("cpu"), s_sd, cfg_s, t_sd, cfg_t, spec_augment=AUG_PARAMS, dropout_seed=7)
    lc = c.forward_backward(x, ids, labels)
    assert torch.equal(x, feats) and not torch.equal(lc, la)
    tm, fm = sr.masks(7, 1, 2, cfg_s.n_mels, 3000, None, AUG_PARAMS)
    pre = torch.from_numpy(sr.apply(feats.numpy(), tm, fm))
    assert torch.equal(c._aug_buf, pre)
    assert torch.equal(lc, DistillationTrainer(RefOps("cpu"), s_sd, cfg_s, t_sd, cfg_t).forward_backward(pre, ids, labels))
    d = DistillationTrainer(RefOps("cpu"), s_sd, cfg_s, t_sd, cfg_t, spec_augment=AUG_PARAMS, dropout_seed=7, augment_teacher=False)
    seen = []
    enc = d.teacher.encode
    d.teacher.encode = lambda f, **k: (seen.append(f.clone()), enc(f, **k))[1]
    ld = d.forward_backward(x, ids, labels)
    assert len(seen) == 1 and torch.equal(seen[0], feats) and torch.equal(d._aug_buf, pre)
    assert torch.equal(ld[0], lc[0]) and not torch.equal(ld[1], lc[1])               # same student CE, another KL


def test_resumed_trainer_continues_the_mask_sequence_and_dropout_masks_stay():
    cfg_t, t_sd, cfg_s, s_sd, feats, ids, labels = micro(seed=4)
    kw = dict(spec_augment=AUG_PARAMS, dropout_seed=7, lr=1e-3)
    a = DistillationTrainer(RefOps("cpu"), s_sd, cfg_s, t_sd, cfg_t, **kw)
    for _ in range(2):
        a.train_step(feats, ids, labels)
    state = a.state_dict()
    assert state["dropout"] == {"dropout": 0.0, "activation_dropout": 0.0, "seed": 7, "step": 2,
                                "spec_augment": sa.normalise(AUG_PARAMS), "augment_teacher": True}
    la = a.train_step(feats, ids, labels)
    b = DistillationTrainer(RefOps("cpu"), s_sd, cfg_s, t_sd, cfg_t)          # resumed: everything comes from the state
    b.load_state_dict(state)
    lb = b.train_step(feats, ids, labels)
    assert torch.equal(la, lb) and torch.equal(a.student_store.P, b.student_store.P)
    assert int(b.student.drop_state.item()) == 3
    tm, fm = sr.masks(7, 3, 2, cfg_s.n_mels, 3000, None, AUG_PARAMS)
    assert torch.equal(b._aug_buf, torch.from_numpy(sr.apply(feats.numpy(), tm, fm)))
    # dropout's masks do not depend on SpecAugment
    masks = []
    for extra in (dict(), dict(spec_augment=AUG_PARAMS)):
        t = DistillationTrainer(dr.DropRefOps("cpu"), s_sd, cfg_s, t_sd, cfg_t, dropout=0.1, activation_dropout=0.05,
                                dropout_seed=7, **extra)
        t.student.keep_masks = {}
        t.forward_backward(feats, ids, labels)
        masks.append(dict(t.student.keep_masks))
    plain, both = masks
    assert set(both) == set(plain) | {sr.SITE_TIME, sr.SITE_FEATURE} and len(plain) > 5 and max(plain) < 512
    for site, m in plain.items():
        assert torch.equal(m, both[site]), site
    assert np.array_equal(both[sr.SITE_TIME].numpy().astype(bool), sr.masks(7, 1, 2, cfg_s.n_mels, 3000, None, AUG_PARAMS)[0])


# ---- 6. the C entry's argument errors (no GPU is touched) --------------------------------------------------------------------
def test_argument_errors_are_rejected_without_touching_the_gpu():
    from distil_whisper_amd import build, ops_hip
    build.build()
    lib = ops_hip.load_library()
    assert "dw_spec_augment" in ops_hip.EXPORTED_SYMBOLS
    buf = torch.zeros(2 * 80 * 64 + 8)
    st = torch.zeros(1, dtype=torch.int64)
    p, s = buf.data_ptr(), st.data_ptr()
    assert lib.dw_spec_augment(None, p, 2, 80, 64, None, 0.1, 10, 2, 0.0, 10, 0, 1, s, None, None, None) == -1      # null in
    assert lib.dw_spec_augment(p, None, 2, 80, 64, None, 0.1, 10, 2, 0.0, 10, 0, 1, s, None, None, None) == -1      # null out
    assert lib.dw_spec_augment(p, p, 2, 80, 64, None, 0.1, 0, 2, 0.0, 10, 0, 1, s, None, None, None) == -1          # mask_length < 1
    assert lib.dw_spec_augment(p, p, 2, 80, 64, None, 0.1, 65, 2, 0.0, 10, 0, 1, s, None, None, None) == -1         # > T
    assert lib.dw_spec_augment(p, p, 2, 80, 64, None, 0.0, 10, 2, 0.1, 81, 0, 1, s, None, None, None) == -1         # > n_mels
    assert lib.dw_spec_augment(p, p, 2, 80, 64, None, 0.1, 10, 2, 0.0, 10, 0, 1, None, None, None, None) == -1      # null step
    assert lib.dw_spec_augment(p, p, 65535, 80, 64, None, 0.1, 10, 2, 0.0, 10, 0, 1, s, None, None, None) == -2     # too many rows
    assert not buf.any()
