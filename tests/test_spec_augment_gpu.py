"""csrc/spec_augment.hip on the MI355X: the kernel against the numpy restatement (tests/spec_augment_restatement.py) bit for bit
over the case matrix, the device-resident step counter (tick, graph replays), the drop-in module and the trainer with
SpecAugment against the same objects without it fed the pre-masked features.

Equality of two training steps: losses, logits and the weight-matrix gradients (their GEMMs store) are compared bit for bit.
Biases, LayerNorm parameters and embeddings are accumulated with float atomics, whose summation order differs between two
runs of the SAME path (tests/test_dropout_gpu.py test_zero_probabilities_are_the_trainer_without_the_arguments measured 3.7e-9
absolute between two identical steps), so they are held per tensor to the 1e-5 relative that test grants that summation order."""
import numpy as np
import pytest
import torch

import spec_augment_restatement as sr
from oracle import whisper_oracle as wo

pytestmark = pytest.mark.gpu

SEED = 0x1234567_89ABCDEF
B = 5
AUG = dict(apply_spec_augment=True, mask_time_prob=0.1, mask_time_length=10, mask_time_min_masks=2, mask_feature_prob=0.2,
           mask_feature_length=3, mask_feature_min_masks=1)
AUG_PARAMS = {k: v for k, v in AUG.items() if k != "apply_spec_augment"}


def relerr(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


@pytest.fixture(scope="module")
def ops():
    from distil_whisper_amd.ops_hip import HipOps
    return HipOps("cuda:0")


def _features(n_mels, T, seed=0, rows=B):
    x = torch.randn(rows, n_mels, T, generator=torch.Generator().manual_seed(seed))
    x[x == 0] = 1.0                    # a zero in the output is a masked element
    return x


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def _params(tc, fc):
    return dict(mask_time_prob=tc[2], mask_time_length=tc[1], mask_time_min_masks=tc[3],
                mask_feature_prob=fc[2], mask_feature_length=fc[1], mask_feature_min_masks=fc[3])


# T = 3000 takes the kernel's 16-byte path, T = 202 (not a multiple of 4) the scalar one; 80 / 128 mel bins are 20 / 32 workgroups per row
@pytest.mark.parametrize("T,n_mels", [(3000, 80), (202, 128)])
def test_kernel_equals_the_restatement_on_the_case_matrix(ops, T, n_mels):
    tcs = [c for c in sr.TIME_CASES if c[0] == T]
    fcs = [c for c in sr.FEATURE_CASES if c[0] == n_mels]
    assert len(tcs) == len(fcs) == 11
    x = _features(n_mels, T, seed=T)
    xd = x.cuda()
    lens = sr.time_lengths(T)
    lens_d = torch.tensor(lens, dtype=torch.int32, device="cuda")
    n = 0
    for tc, fc in zip(tcs, fcs):
        p = _params(tc, fc)
        for step in sr.STEPS:
            wt, wf = sr.masks(SEED, step, B, n_mels, T, lens, p)
            want = sr.apply(x.numpy(), wt, wf).view(np.int32)
            st = ops.dropout_state(step)
            out, tm, fm = ops.spec_augment(xd, SEED, st, p, lengths=lens_d, out=torch.full_like(xd, float("nan")), want_masks=True)
            assert np.array_equal(tm.cpu().numpy().astype(bool), wt), (tc, step)
            assert np.array_equal(fm.cpu().numpy().astype(bool), wf), (fc, step)
            assert np.array_equal(_bits(out), want), (tc, fc, step)          # zeros exactly where masked, the input's bits elsewhere
            y = xd.clone()
            same, no_tm, no_fm = ops.spec_augment(y, SEED, st, p, lengths=lens_d)          # in place, no mask outputs
            assert same is y and no_tm is None and no_fm is None and np.array_equal(_bits(y), want), (tc, fc, step)
            assert np.array_equal(_bits(xd), _bits(x))                      # the out-of-place input is left alone
            n += 1
    assert n == 33
    # no lengths: every row is T long
    p = _params(tcs[4], fcs[4])
    wt, wf = sr.masks(SEED, 7, B, n_mels, T, None, p)
    y = xd.clone()
    ops.spec_augment(y, SEED, ops.dropout_state(7), p)
    assert np.array_equal(_bits(y), sr.apply(x.numpy(), wt, wf).view(np.int32))
    # one axis only
    for q in (dict(p, mask_time_prob=0.0), dict(p, mask_feature_prob=0.0)):
        wt, wf = sr.masks(SEED, 7, B, n_mels, T, lens, q)
        assert not (wt.any() and wf.any())
        out, tm, fm = ops.spec_augment(xd, SEED, ops.dropout_state(7), q, lengths=lens_d, out=torch.empty_like(xd), want_masks=True)
        assert np.array_equal(tm.cpu().numpy().astype(bool), wt) and np.array_equal(fm.cpu().numpy().astype(bool), wf)
        assert np.array_equal(_bits(out), sr.apply(x.numpy(), wt, wf).view(np.int32))


def test_unaligned_planes_odd_mel_count_and_argument_errors(ops):
    """A plane that starts 4 bytes off a 16-byte boundary takes the scalar path at T % 4 == 0; 83 mel bins leave a last workgroup
    with three rows; argument errors come back as -1 without a launch."""
    T, n_mels = 3000, 83
    p = dict(AUG_PARAMS, mask_time_prob=0.3)
    x = _features(n_mels, T, seed=3, rows=2)
    flat = torch.full((2 * n_mels * T + 2,), float("nan"), device="cuda")
    xd = flat[1:-1].view(2, n_mels, T)
    xd.copy_(x)
    wt, wf = sr.masks(SEED, 5, 2, n_mels, T, None, p)
    st = ops.dropout_state(5)
    out, tm, fm = ops.spec_augment(xd, SEED, st, p, want_masks=True)
    assert np.array_equal(tm.cpu().numpy().astype(bool), wt) and np.array_equal(fm.cpu().numpy().astype(bool), wf)
    assert np.array_equal(_bits(xd), sr.apply(x.numpy(), wt, wf).view(np.int32))
    assert torch.isnan(flat[0]) and torch.isnan(flat[-1])                    # nothing outside the planes is written
    lib, ptr, s = ops.lib, xd.data_ptr(), st.data_ptr()
    assert lib.dw_spec_augment(None, ptr, 2, n_mels, T, None, 0.1, 10, 2, 0.0, 10, 0, 1, s, None, None, None) == -1
    assert lib.dw_spec_augment(ptr, None, 2, n_mels, T, None, 0.1, 10, 2, 0.0, 10, 0, 1, s, None, None, None) == -1
    assert lib.dw_spec_augment(ptr, ptr, 2, n_mels, T, None, 0.1, 0, 2, 0.0, 10, 0, 1, s, None, None, None) == -1
    assert lib.dw_spec_augment(ptr, ptr, 2, n_mels, T, None, 0.1, T + 1, 2, 0.0, 10, 0, 1, s, None, None, None) == -1
    assert lib.dw_spec_augment(ptr, ptr, 2, n_mels, T, None, 0.1, 10, 2, 0.1, n_mels + 1, 0, 1, s, None, None, None) == -1
    with pytest.raises(ValueError, match="`mask_length` has to be bigger than 0."):
        ops.spec_augment(xd, SEED, st, dict(p, mask_time_length=0))
    assert np.array_equal(_bits(xd), sr.apply(x.numpy(), wt, wf).view(np.int32))          # the rejected calls wrote nothing


def test_step_counter_tick_and_graph_replays(ops):
    T, n_mels, s = 3000, 80, 2**32 - 1             # the tick carries into the high word
    p = dict(AUG_PARAMS)
    x = _features(n_mels, T, seed=9, rows=2).cuda()
    st = ops.dropout_state(s)
    _, tm0, _ = ops.spec_augment(x, SEED, st, p, out=torch.empty_like(x), want_masks=True)
    ops.dropout_tick(st)
    _, tm1, fm1 = ops.spec_augment(x, SEED, st, p, out=torch.empty_like(x), want_masks=True)
    want = [sr.masks(SEED, s + i, 2, n_mels, T, None, p) for i in range(4)]
    assert np.array_equal(tm0.cpu().numpy().astype(bool), want[0][0]) and np.array_equal(tm1.cpu().numpy().astype(bool), want[1][0])
    assert np.array_equal(fm1.cpu().numpy().astype(bool), want[1][1]) and not np.array_equal(want[0][0], want[1][0])
    # one tick + one launch captured on a single stream: every replay draws the next step's masks
    out = torch.empty_like(x)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.dropout_tick(st)
        _, tm, fm = ops.spec_augment(x, SEED, st, p, out=out, want_masks=True)
    for i in (2, 3):
        graph.replay()
        torch.cuda.synchronize()
        assert int(st.item()) == s + i
        assert np.array_equal(tm.cpu().numpy().astype(bool), want[i][0]) and np.array_equal(fm.cpu().numpy().astype(bool), want[i][1])
        assert np.array_equal(_bits(out), sr.apply(x.cpu().numpy(), *want[i]).view(np.int32))
    assert not np.array_equal(want[2][0], want[3][0])


# ---- the drop-in module and the trainer -----------------------------------------------------------------------------------------
def _setup(Bt=2, T=40):
    cfg_t = wo.CONFIGS["micro"]
    t_sd = wo.init_state_dict(cfg_t, 31)
    s_sd, cfg_s = wo.student_from_teacher(t_sd, cfg_t, 2, 1)
    b = wo.synthetic_batch(cfg_t, Bt, seed=32, T=T, with_audio=False)
    feats = (torch.randn(Bt, cfg_t.n_mels, 3000, generator=torch.Generator().manual_seed(1)) * 0.5).cuda()
    return cfg_t, t_sd, cfg_s, s_sd, feats, b["decoder_input_ids"].cuda(), b["labels"].cuda()


def _config(cfg, **kw):
    from distil_whisper_amd.modeling import WhisperConfig
    return WhisperConfig(vocab_size=cfg.vocab, num_mel_bins=cfg.n_mels, d_model=cfg.d_model, encoder_layers=cfg.enc_layers,
                         decoder_layers=cfg.dec_layers, encoder_attention_heads=cfg.heads, decoder_attention_heads=cfg.heads,
                         encoder_ffn_dim=cfg.ffn, decoder_ffn_dim=cfg.ffn, pad_token_id=cfg.pad_token_id, bos_token_id=0,
                         eos_token_id=0, decoder_start_token_id=cfg.decoder_start_token_id, **kw)


def _same_gradients(sa_store, sb_store):
    """weight matrices bit for bit, the atomically summed tensors within 1e-5 relative (see the module docstring)"""
    exact, worst = 0, 0.0
    for n, (_, _, kind) in sa_store.entries.items():
        if n not in sa_store.g:
            continue
        if kind == "w":
            assert torch.equal(sa_store.g[n], sb_store.g[n]), n
            exact += 1
        else:
            e = relerr(sb_store.g[n], sa_store.g[n])
            worst = max(worst, e)
            assert e < 1e-5, (n, e)
    print("worst relative difference of an atomically summed tensor", worst)
    assert exact > 20


def test_drop_in_masks_in_training_mode_only(ops):
    from distil_whisper_amd.modeling import WhisperForConditionalGeneration
    _, _, cfg_s, s_sd, feats, ids, labels = _setup()
    seed, lens = 5, [3000, 1777]
    am = (torch.arange(3000, device="cuda")[None, :] < torch.tensor(lens, device="cuda")[:, None]).long()
    tm, fm = sr.masks(seed, 1, 2, cfg_s.n_mels, 3000, lens, AUG_PARAMS)          # the first training forward is step 1
    pre = torch.from_numpy(sr.apply(feats.cpu().numpy(), tm, fm)).cuda()
    assert not torch.equal(pre, feats)
    on = WhisperForConditionalGeneration(_config(cfg_s, **AUG), ops=ops, state_dict=s_sd, dropout_seed=seed)
    off = WhisperForConditionalGeneration(_config(cfg_s), ops=ops, state_dict=s_sd)
    on.train()
    off.train()
    x = feats.clone()
    a = on(input_features=x, attention_mask=am, decoder_input_ids=ids, labels=labels)
    a.loss.backward()
    b = off(input_features=pre.clone(), decoder_input_ids=ids, labels=labels)
    b.loss.backward()
    assert torch.equal(x, pre)                                                   # masked in place, as the reference leaves it
    assert torch.equal(a.loss, b.loss) and torch.equal(torch.as_tensor(a.logits), torch.as_tensor(b.logits))
    assert torch.equal(a.encoder_last_hidden_state, b.encoder_last_hidden_state)
    _same_gradients(on.store, off.store)
    assert int(on.engine.drop_state.item()) == 1
    # eval mode, generate and encoder_outputs leave the features and the counter alone
    on.eval()
    x = feats.clone()
    with torch.no_grad():
        e = on(input_features=x, attention_mask=am, decoder_input_ids=ids, labels=labels)
        want = off(input_features=feats.clone(), decoder_input_ids=ids, labels=labels)
        on.generate(x, max_new_tokens=4)
    assert torch.equal(x, feats) and torch.equal(e.loss, want.loss) and int(on.engine.drop_state.item()) == 1
    on.train()
    on.generate(x, max_new_tokens=4)
    on(encoder_outputs=(want.encoder_last_hidden_state,), decoder_input_ids=ids, labels=labels)
    assert torch.equal(x, feats)


def test_trainer_masks_into_its_own_buffer(ops):
    from distil_whisper_amd.distill import DistillationTrainer
    cfg_t, t_sd, cfg_s, s_sd, feats, ids, labels = _setup()
    tm, fm = sr.masks(7, 1, 2, cfg_s.n_mels, 3000, None, AUG_PARAMS)
    pre = torch.from_numpy(sr.apply(feats.cpu().numpy(), tm, fm)).cuda()
    x = feats.clone()
    plain = DistillationTrainer(ops, s_sd, cfg_s, t_sd, cfg_t)
    lp = plain.forward_backward(pre, ids, labels).clone()
    aug = DistillationTrainer(ops, s_sd, cfg_s, t_sd, cfg_t, spec_augment=AUG_PARAMS, dropout_seed=7)
    la = aug.forward_backward(x, ids, labels).clone()
    assert torch.equal(x, feats) and torch.equal(aug._aug_buf, pre)              # the caller's tensor is never written
    assert torch.equal(la, lp)
    _same_gradients(aug.student_store, plain.student_store)
    # the teacher on the clean features: with kl_weight = 0 the student's loss and gradients are still those of the pre-masked run
    p0 = DistillationTrainer(ops, s_sd, cfg_s, t_sd, cfg_t, kl_weight=0.0)
    l0 = p0.forward_backward(pre, ids, labels).clone()
    clean = DistillationTrainer(ops, s_sd, cfg_s, t_sd, cfg_t, spec_augment=AUG_PARAMS, dropout_seed=7, augment_teacher=False,
                                kl_weight=0.0)
    seen, enc = [], clean.teacher.encode
    clean.teacher.encode = lambda f, **k: (seen.append(f.clone()), enc(f, **k))[1]
    lc = clean.forward_backward(x, ids, labels).clone()
    assert len(seen) == 1 and torch.equal(seen[0], feats) and torch.equal(x, feats)
    assert torch.equal(lc[0], l0[0]) and torch.equal(lc[2], l0[2])
    _same_gradients(clean.student_store, p0.student_store)


def test_graph_replays_use_fresh_masks(ops):
    from distil_whisper_amd.distill import DistillationTrainer
    cfg_t, t_sd, cfg_s, s_sd, feats, ids, labels = _setup()
    g = DistillationTrainer(ops, s_sd, cfg_s, t_sd, cfg_t, spec_augment=AUG_PARAMS, dropout_seed=5)
    g.student.keep_masks = {}
    seen = []
    for i in range(3):
        g.train_step_graphed(feats, ids, labels, eager_steps=1)
        torch.cuda.synchronize()
        assert (g._graph["graph"] is not None) == (i >= 1)
        step = int(g.student.drop_state.item())
        assert step == i + 1
        if i >= 1:
            tm, fm = sr.masks(5, step, 2, cfg_s.n_mels, 3000, None, AUG_PARAMS)
            assert np.array_equal(g.student.keep_masks[sr.SITE_TIME].cpu().numpy().astype(bool), tm)
            assert np.array_equal(g.student.keep_masks[sr.SITE_FEATURE].cpu().numpy().astype(bool), fm)
            assert np.array_equal(_bits(g._aug_buf), sr.apply(feats.cpu().numpy(), tm, fm).view(np.int32))
            seen.append(tm)
    assert not np.array_equal(seen[0], seen[1])
