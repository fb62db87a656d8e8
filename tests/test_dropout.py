"""Training-mode `dropout` / `activation_dropout` without a GPU: the mask generator's restatement against known answers
and its statistics, the drop-in module and the trainer over the torch restatement of the dropout kernels
(tests/dropout_restatement.py DropRefOps) against `transformers` fed the same masks, and the bookkeeping around them
(eval mode, p = 0, config round trip, trainer state)."""
import math

import numpy as np
import pytest
import torch

import dropout_restatement as dr
from distil_whisper_amd.distill import DistillationTrainer
from distil_whisper_amd.engine import WhisperEngine
from distil_whisper_amd.modeling import WhisperConfig, WhisperForConditionalGeneration
from oracle import whisper_oracle as wo
from oracle.ref_ops import RefOps


def relerr(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-30)).item()


# ---- 1. known answers ---------------------------------------------------------------------------------------------------
# counter / key -> output of Philox4x32-10.  The first and the third are the Random123 known-answer vectors as quoted in the
# feature request.  Of the second (all ones) the request quotes the third word as a20bc7c9: the round function of the paper,
# evaluated with plain Python integers and independently with the numpy restatement, gives a20bc7c6 -- the other eleven
# quoted words agree, which an implementation error could not leave standing -- so the quoted word is taken as mis-remembered.
KAT = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


def _philox_ints(c, k):
    """the paper's round function with Python integers (no numpy): an independent derivation for the vectors above"""
    c, k = list(c), list(k)
    for _ in range(10):
        p0, p1 = dr.M0 * c[0], dr.M1 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + dr.W0) & 0xFFFFFFFF, (k[1] + dr.W1) & 0xFFFFFFFF]
    return c


@pytest.mark.parametrize("counter,key,want", KAT)
def test_philox_known_answers(counter, key, want):
    got = " ".join("%08x" % int(x) for x in dr.philox4x32_10(counter, key))
    assert got == want
    assert " ".join("%08x" % x for x in _philox_ints(counter, key)) == want


def test_philox_vectorised_equals_scalar():
    rng = np.random.default_rng(0)
    c = rng.integers(0, 2**32, size=(4, 5), dtype=np.uint64)
    out = dr.philox4x32_10(tuple(c), (7, 9))
    for i in range(5):
        assert [int(w[i]) for w in out] == _philox_ints([int(x) for x in c[:, i]], (7, 9))


# ---- 2. statistics ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.05, 0.1, 0.5])
def test_keep_rate_and_mask_identity(p):
    rows, cols = 1024, 1024
    N = rows * cols
    m = dr.mask(11, 3, 5, rows, cols, p)
    thr = dr.threshold(p)
    print("kept", m.sum() / N, "expected", 1 - thr / 2**32)
    assert abs(m.sum() / N - (1 - thr / 2**32)) < 5 * math.sqrt(p * (1 - p) / N)
    small = dr.mask(11, 3, 5, 64, cols, p)
    assert np.array_equal(small, m[:64])                            # same triple, same mask (rows are a prefix)
    assert not np.array_equal(small, dr.mask(11, 3, 6, 64, cols, p))  # another site
    assert not np.array_equal(small, dr.mask(11, 4, 5, 64, cols, p))  # another step
    assert not np.array_equal(small, dr.mask(12, 3, 5, 64, cols, p))  # another seed
    assert not np.array_equal(small, dr.mask(11, 3 + 2**32, 5, 64, cols, p))  # the high word of the step counts
    assert np.array_equal(dr.unpack_mask(dr.pack_mask(small), cols), small)
    assert dr.pack_mask(small)[0, 0] == sum(int(small[0, j]) << j for j in range(8))


def test_threshold_edges():
    assert dr.threshold(0.0) == 0 and dr.mask(1, 1, 1, 8, 64, 0.0).all()
    assert dr.threshold(0.5) == 2**31 and dr.threshold(1 - 2**-40) == 2**32 - 1


# ---- 3. the drop-in against transformers with the same masks -----------------------------------------------------------
def micro(seed=9, B=2, T=13):
    cfg_t = wo.CONFIGS["micro"]
    t_sd = wo.init_state_dict(cfg_t, seed)
    s_sd, cfg_s = wo.student_from_teacher(t_sd, cfg_t, 2, 1)
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn(B, cfg_s.n_mels, 3000, generator=g) * 0.5
    b = wo.synthetic_batch(cfg_s, B, seed=seed + 1, T=T, with_audio=False)
    return cfg_t, t_sd, cfg_s, s_sd, feats, b["decoder_input_ids"], b["labels"]


def config_of(cfg, **kw):
    return WhisperConfig(vocab_size=cfg.vocab, num_mel_bins=cfg.n_mels, d_model=cfg.d_model, encoder_layers=cfg.enc_layers,
                         decoder_layers=cfg.dec_layers, encoder_attention_heads=cfg.heads, decoder_attention_heads=cfg.heads,
                         encoder_ffn_dim=cfg.ffn, decoder_ffn_dim=cfg.ffn, pad_token_id=cfg.pad_token_id, bos_token_id=0,
                         eos_token_id=0, decoder_start_token_id=cfg.decoder_start_token_id, **kw)


def hf_sites(cfg, p_drop, p_act):
    """the order in which transformers' Whisper calls nn.functional.dropout, as (site, columns, p)"""
    site, D, Fd = WhisperEngine.drop_site, cfg.d_model, cfg.ffn
    out = [(site(0, -1, 0), D, p_drop)]
    for i in range(cfg.enc_layers):
        out += [(site(0, i, 0), D, p_drop), (site(0, i, 3), Fd, p_act), (site(0, i, 2), D, p_drop)]
    out.append((site(1, -1, 0), D, p_drop))
    for i in range(cfg.dec_layers):
        out += [(site(1, i, 0), D, p_drop), (site(1, i, 1), D, p_drop), (site(1, i, 3), Fd, p_act), (site(1, i, 2), D, p_drop)]
    return [e for e in out if e[2] > 0]         # (calls with p == 0 pass through)


def test_site_numbers_are_unique():
    s = WhisperEngine.drop_site
    all_sites = [s(side, layer, kind) for side in (0, 1) for layer in range(-1, 32) for kind in range(4)]
    assert len(set(all_sites)) == len(all_sites) and min(all_sites) >= 0


@pytest.mark.parametrize("p_drop,p_act", [(0.1, 0.05), (0.1, 0.0), (0.0, 0.1)])
def test_drop_in_train_mode_matches_transformers_with_the_same_masks(p_drop, p_act):
    import transformers
    _, _, cfg_s, s_sd, feats, ids, labels = micro()
    seed = 5
    model = WhisperForConditionalGeneration(config_of(cfg_s, dropout=p_drop, activation_dropout=p_act),
                                            ops=dr.DropRefOps("cpu", lowp=torch.float32), state_dict=s_sd, dropout_seed=seed)
    model.train()
    hc = transformers.WhisperConfig(vocab_size=cfg_s.vocab, num_mel_bins=cfg_s.n_mels, d_model=cfg_s.d_model,
                                    encoder_layers=cfg_s.enc_layers, decoder_layers=cfg_s.dec_layers,
                                    encoder_attention_heads=cfg_s.heads, decoder_attention_heads=cfg_s.heads,
                                    encoder_ffn_dim=cfg_s.ffn, decoder_ffn_dim=cfg_s.ffn, pad_token_id=cfg_s.pad_token_id,
                                    bos_token_id=0, eos_token_id=0, decoder_start_token_id=cfg_s.decoder_start_token_id,
                                    dropout=p_drop, activation_dropout=p_act)
    hf = transformers.WhisperForConditionalGeneration(hc).float()
    hf.load_state_dict(model.state_dict())
    hf.train()
    with dr.patched_dropout(seed, 1, hf_sites(cfg_s, p_drop, p_act)) as left:      # the first training forward is step 1
        ref = hf(input_features=feats, decoder_input_ids=ids, labels=labels)
        assert not left, "transformers made fewer dropout calls than the engine has sites"
    ref.loss.backward()
    out = model(input_features=feats, decoder_input_ids=ids, labels=labels)
    print("loss", out.loss.item(), "reference", ref.loss.item())
    assert abs(out.loss.item() - ref.loss.item()) < 2e-5 * abs(ref.loss.item())
    out.loss.backward()
    # and the masks matter: without them the loss is another one
    hf.eval()
    with torch.no_grad():
        plain = hf(input_features=feats, decoder_input_ids=ids, labels=labels).loss
    assert abs(plain.item() - ref.loss.item()) > 1e-3 * abs(ref.loss.item())
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


# ---- 4. eval mode, p = 0, teacher, eval_step ---------------------------------------------------------------------------
def test_eval_mode_and_zero_probability_change_nothing():
    cfg_t, t_sd, cfg_s, s_sd, feats, ids, labels = micro()
    plain = WhisperForConditionalGeneration(config_of(cfg_s), ops=RefOps("cpu"), state_dict=s_sd)
    want = plain(input_features=feats, decoder_input_ids=ids, labels=labels)
    want.loss.backward()
    ops = dr.DropRefOps("cpu")
    dropped = WhisperForConditionalGeneration(config_of(cfg_s, dropout=0.1, activation_dropout=0.05), ops=ops, state_dict=s_sd)
    dropped.eval()
    got = dropped(input_features=feats, decoder_input_ids=ids, labels=labels)
    got.loss.backward()
    assert torch.equal(got.loss, want.loss) and torch.equal(torch.as_tensor(got.logits), torch.as_tensor(want.logits))
    for (n, a), (_, b) in zip(dropped.named_parameters(), plain.named_parameters()):
        assert (a.grad is None and b.grad is None) or torch.equal(a.grad, b.grad), n
    assert int(dropped.engine.drop_state.item()) == 0           # no step was drawn
    dropped.train()
    tr_loss = dropped(input_features=feats, decoder_input_ids=ids, labels=labels).loss
    assert not torch.equal(tr_loss, want.loss) and int(dropped.engine.drop_state.item()) == 1
    zero = WhisperForConditionalGeneration(config_of(cfg_s, dropout=0.0, activation_dropout=0.0), ops=ops, state_dict=s_sd)
    zero.train()
    z = zero(input_features=feats, decoder_input_ids=ids, labels=labels)
    assert torch.equal(z.loss, want.loss) and zero.engine.drop_state is None
    # an inference-only bf16 model ignores the fields
    bf = WhisperForConditionalGeneration(config_of(cfg_s, dropout=0.1), ops=ops, state_dict=s_sd, dtype=torch.bfloat16)
    assert bf.engine.p_drop == 0.0

    # trainer: probabilities 0 = a trainer built without the arguments; eval_step and the teacher never drop
    a = DistillationTrainer(RefOps("cpu"), s_sd, cfg_s, t_sd, cfg_t)
    b = DistillationTrainer(ops, s_sd, cfg_s, t_sd, cfg_t, dropout=0.0, activation_dropout=0.0, dropout_seed=3)
    c = DistillationTrainer(ops, s_sd, cfg_s, t_sd, cfg_t, dropout=0.1, activation_dropout=0.1)
    la, lb = a.forward_backward(feats, ids, labels), b.forward_backward(feats, ids, labels)
    assert torch.equal(la, lb) and torch.equal(a.student_store.G, b.student_store.G)
    assert "dropout" not in b.state_dict() and set(a.state_dict()) == set(b.state_dict())
    assert torch.equal(a.eval_step(feats, ids, labels), c.eval_step(feats, ids, labels))
    assert c.teacher.p_drop == 0.0 and c.teacher.p_act == 0.0 and not c.teacher.training
    lc = c.forward_backward(feats, ids, labels)
    assert not torch.equal(lc, la) and torch.isfinite(c.student_store.G).all()
    assert torch.equal(a.eval_step(feats, ids, labels), c.eval_step(feats, ids, labels))   # also after a training step
    # ops without the kernels: an error, never a silent pass without dropout
    with pytest.raises(RuntimeError, match="no dropout kernels"):
        DistillationTrainer(RefOps("cpu"), s_sd, cfg_s, t_sd, cfg_t, dropout=0.1)


# ---- 5. config ----------------------------------------------------------------------------------------------------------
def test_config_round_trip_and_unbuilt_options(tmp_path):
    cfg = WhisperConfig(dropout=0.1, activation_dropout=0.05)
    cfg.save_pretrained(str(tmp_path))
    back = WhisperConfig.from_pretrained(str(tmp_path))
    assert back.dropout == 0.1 and back.activation_dropout == 0.05
    for kw in (dict(attention_dropout=0.1), dict(encoder_layerdrop=0.1), dict(decoder_layerdrop=0.1), dict(scale_embedding=True)):
        with pytest.raises(ValueError, match="not implemented.*builds `dropout` and `activation_dropout`"):
            WhisperConfig(**kw)
    for kw in (dict(dropout=1.0), dict(activation_dropout=-0.1)):
        with pytest.raises(ValueError, match=r"\[0, 1\)"):
            WhisperConfig(**kw)
    # through the model
    _, _, cfg_s, s_sd, *_ = micro()
    model = WhisperForConditionalGeneration(config_of(cfg_s, dropout=0.1, activation_dropout=0.05), ops=dr.DropRefOps("cpu"),
                                            state_dict=s_sd)
    model.save_pretrained(str(tmp_path / "m"))
    again = WhisperForConditionalGeneration.from_pretrained(str(tmp_path / "m"), ops=dr.DropRefOps("cpu"))
    assert (again.engine.p_drop, again.engine.p_act) == (0.1, 0.05)


# ---- 6. trainer state ---------------------------------------------------------------------------------------------------
def test_resumed_trainer_continues_the_mask_sequence():
    cfg_t, t_sd, cfg_s, s_sd, feats, ids, labels = micro(seed=4)
    kw = dict(dropout=0.1, activation_dropout=0.05, dropout_seed=7, lr=1e-3)
    a = DistillationTrainer(dr.DropRefOps("cpu"), s_sd, cfg_s, t_sd, cfg_t, **kw)
    for _ in range(2):
        a.train_step(feats, ids, labels)
    state = a.state_dict()
    assert state["dropout"] == {"dropout": 0.1, "activation_dropout": 0.05, "seed": 7, "step": 2}
    la = a.train_step(feats, ids, labels)
    b = DistillationTrainer(dr.DropRefOps("cpu"), s_sd, cfg_s, t_sd, cfg_t)         # resumed: everything comes from the state
    b.load_state_dict(state)
    lb = b.train_step(feats, ids, labels)
    assert torch.equal(la, lb) and torch.equal(a.student_store.P, b.student_store.P)
    assert int(b.student.drop_state.item()) == 3
    c = DistillationTrainer(dr.DropRefOps("cpu"), s_sd, cfg_s, t_sd, cfg_t, **kw)   # the sequence matters: step 1's masks differ
    c.student_store.load_state_dict(state["model"])
    assert not torch.equal(c.forward_backward(feats, ids, labels), la)
