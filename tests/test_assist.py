"""Speculative (assisted) decoding on the CPU: the torch round functions of decoding.py against the float64 restatement
(tests/assist_restatement.py) on planted rounds (tests/assist_cases.py), `assisted_greedy_decode` over the torch restatement of
the kernels (oracle.ref_ops: no `assist_*` entries, so the torch functions), and the decoder-only drop-in
`WhisperForCausalLM` against `transformers.WhisperForCausalLM`."""
import json
import os

import numpy as np
import pytest
import torch

from distil_whisper_amd.decoding import assist_accept_torch, assist_pick_torch, assisted_greedy_decode
from oracle import gen_golden_decode as gd
from oracle.ref_ops import RefOps
from tests import assist_cases as ac
from tests.assist_restatement import accept_ref, pick_ref

GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode.json")))


def planted(V, B, k, name, sc):
    """The case of scenario `name` (first seed whose mass-rule margins are clear: assist_cases asserts it)."""
    for seed in range(40):
        try:
            return ac.make_case(1000 * seed + 17 * B + k + len(name), V, B, k, sc)
        except AssertionError:
            continue
    raise AssertionError(f"no clear-margin case for {name}")


def torch_round(c):
    L, k, P0 = c["L"], c["k"], c["P0"]
    tok = torch.from_numpy(c["tokens"])
    V = c["logits"].shape[-1]
    sup = None
    if c["suppress"]:
        sup = torch.zeros(V)
        sup[torch.tensor(c["suppress"])] = float("-inf")
    own = assist_pick_torch(torch.from_numpy(c["logits"]).float(), tok[:, :L + k], L, P0, c["eos"], c["min_new"], sup, c["ts"])
    new, done, n_ok = assist_accept_torch(own.clone(), tok[:, :L + k], L, k, torch.from_numpy(c["done"]), c["eos"], c["fill"])
    return own, new, done, n_ok


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("k", [0, 1, 5])
def test_torch_round_matches_the_restatement_on_planted_rounds(B, k):
    seen = set()
    for name, sc in ac.scenarios(B, k).items():
        c = planted(1030, B, k, name, sc)
        L = c["L"]
        own_ref, _ = pick_ref(c["logits"], c["tokens"], L, c["P0"], c["eos"], c["min_new"], c["suppress"], (), c["ts"])
        assert own_ref.tolist() == c["own"].tolist()
        tok_ref, done_ref, n_ref, _ = accept_ref(own_ref, c["tokens"], L, k, c["done"], c["eos"], c["fill"])
        own, new, done, n_ok = torch_round(c)
        assert own.tolist() == own_ref.tolist(), name
        assert n_ok == n_ref, name
        assert new.tolist() == tok_ref[:, L:L + n_ok + 1].tolist(), name
        assert done.tolist() == done_ref.tolist(), name
        seen.add((name, n_ok))
        # what the scenario is there for
        live = [r for r, d in zip(sc["reject"], sc["done"]) if not d]
        if sc["mass"] is None and not sc["suppress_top"]:
            assert n_ok <= min(live + [k])
        if name in ("all_accepted", "done_row") and live:
            assert n_ok == k, name
        if name == "done_row":
            assert (tok_ref[B - 1, L:L + n_ok + 1] == c["fill"]).all()
        if name == "eos_accepted" and k >= 1:
            assert done_ref.all() and (tok_ref[:, L + 2:L + n_ok + 1] == c["fill"]).all() and (tok_ref[:, L + 1] == c["eos"]).all()
        if name == "min_new_inside":
            assert (own_ref[:, :min(2, k)] != c["eos"]).all() and (k < 2 or (own_ref[:, 2] == c["eos"]).all())
        if name == "ts_mass_taken":
            assert (own_ref[:, 0] >= c["lay"]["tb"]).all()          # (later positions: the pair rules)
        if name == "ts_mass_not_taken":
            assert (own_ref[:, 0] < c["lay"]["tb"]).all()
        if name == "ts_first":
            tb = c["lay"]["tb"]
            assert ((own_ref[:, 0] >= tb) & (own_ref[:, 0] <= tb + 1)).all()
    if k == 5:
        assert {n for n, _ in seen} == set(ac.scenarios(B, k))
        assert ("reject_first", 0) in seen and ("reject_middle", 2) in seen and ("rows_differ", 5 if B == 1 else 1) in seen


def _model(ops, cfg, sd, fields):
    from distil_whisper_amd.generation import GenerationConfig
    from distil_whisper_amd.modeling import WhisperForConditionalGeneration
    m = WhisperForConditionalGeneration(cfg, ops=ops, state_dict=sd)
    m.generation_config = GenerationConfig.from_any(fields)
    return m


def _models(ops, seed, fields):
    sd_t = gd.weights(seed)
    sd_s, cfg_s = gd.student(sd_t)
    return _model(ops, gd.CFG_T, sd_t, fields), _model(ops, cfg_s, sd_s, fields), sd_s, cfg_s


def test_fixture_assistant_scenarios_are_unchanged_on_the_torch_path():
    ops = RefOps("cpu", lowp=torch.float32)
    assert not hasattr(ops, "assist_pick")
    todo = [s for s in GOLD["scenarios"] if s.get("assistant") and s.get("kind") == "short" and not s.get("use_encoder_outputs")]
    assert todo
    for s in todo:
        teacher, student, _, _ = _models(ops, s["seed"], s["generation_config"])
        model = teacher if s["model"] == "teacher" else student
        f = gd.features(s["seed"] + 1, s["B"])
        got = model.generate(f, assistant_model=student, return_dict_in_generate=True, **s["gen_kwargs"]).sequences
        assert got.tolist() == s["sequences"], s["name"]
        plain = model.generate(f, return_dict_in_generate=True, **s["gen_kwargs"]).sequences      # the target's own greedy tokens
        assert got.tolist() == plain.tolist()


# ---- WhisperForCausalLM ---------------------------------------------------------------------------------------------------------
def relerr(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-30)).item()


def _hf_config(**kw):
    import transformers
    base = dict(vocab_size=120, num_mel_bins=8, encoder_layers=1, encoder_attention_heads=2, decoder_layers=2,
                decoder_attention_heads=2, decoder_ffn_dim=96, encoder_ffn_dim=96, d_model=128, max_source_positions=20,
                max_target_positions=24, pad_token_id=1, bos_token_id=1, eos_token_id=1, decoder_start_token_id=2,
                suppress_tokens=None, begin_suppress_tokens=None)
    base.update(kw)
    return transformers.WhisperConfig(**base)


def test_causal_lm_matches_transformers(tmp_path):
    import transformers
    from distil_whisper_amd import WhisperForCausalLM
    torch.manual_seed(0)
    ops = RefOps("cpu", lowp=torch.float32)
    ref = transformers.WhisperForCausalLM(_hf_config()).eval()
    ref.save_pretrained(tmp_path / "dec")
    m = WhisperForCausalLM.from_pretrained(str(tmp_path / "dec"), ops=ops)
    theirs = ref.state_dict()
    assert set(m.state_dict()) == set(theirs) and not any(k.startswith("model.encoder.") for k in m.state_dict())
    assert not any(n.startswith("model.encoder.") for n in m.store.entries)            # nothing of an encoder in the flat store
    assert sum(p.numel() for p in m.parameters()) == sum(p.numel() for p in ref.parameters())
    assert m.proj_out.weight is m.model.decoder.embed_tokens.weight
    ids, enc = torch.randint(0, 120, (2, 7)), torch.randn(2, 20, 128)
    with torch.no_grad():
        want = ref(input_ids=ids, encoder_outputs=(enc,), use_cache=False).logits
    got = m(input_ids=ids, encoder_outputs=(enc,)).logits
    assert got.shape == want.shape and relerr(got, want) < 1e-5
    # a full checkpoint: the decoder tensors are taken, the encoder is dropped
    full = transformers.WhisperForConditionalGeneration(_hf_config()).eval()
    full.save_pretrained(tmp_path / "full")
    mf = WhisperForCausalLM.from_pretrained(str(tmp_path / "full"), ops=ops)
    assert set(mf.state_dict()) == set(theirs)
    with torch.no_grad():
        want_f = full.model.decoder(input_ids=ids, encoder_hidden_states=enc, use_cache=False).last_hidden_state @ \
            full.proj_out.weight.T
    assert relerr(mf(input_ids=ids, encoder_outputs=enc).logits, want_f) < 1e-5
    # save_pretrained -> from_pretrained is the identity
    m.save_pretrained(str(tmp_path / "again"))
    m2 = WhisperForCausalLM.from_pretrained(str(tmp_path / "again"), ops=ops)
    a, b = m.state_dict(), m2.state_dict()
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
    with pytest.raises(NotImplementedError):
        m.generate(enc)


def test_causal_lm_assistant_equals_the_full_student_sharing_the_encoder():
    from distil_whisper_amd import WhisperForCausalLM
    from distil_whisper_amd.generation import GenerationConfig
    ops = RefOps("cpu", lowp=torch.float32)
    seed = 310
    fields = gd.generation_fields(multilingual=True, suppress=True, timestamps=True)
    teacher, student, sd_s, cfg_s = _models(ops, seed, fields)
    full = _model(ops, cfg_s, {**sd_s, **{k: v for k, v in teacher.state_dict().items() if k.startswith("model.encoder.")}}, fields)
    full.share_encoder_output = True
    causal = WhisperForCausalLM(cfg_s, ops=ops, state_dict=sd_s)
    causal.generation_config = GenerationConfig.from_any(fields)
    assert not hasattr(causal, "share_encoder_output")
    one = gd.features(seed + 5, 2)
    long1 = torch.cat([gd.features(seed + 1, 1), gd.features(seed + 2, 1)[..., :2200]], -1)
    for feats, kw in ((one, dict(max_new_tokens=7, language="en")),                                   # a single window
                      (long1, dict(max_new_tokens=6, return_timestamps=True, language="en"))):      # the seek loop
        want = teacher.generate(feats, assistant_model=full, **kw)
        stats = (teacher.last_drafted, teacher.last_accepted)
        got = teacher.generate(feats, assistant_model=causal, **kw)
        assert got.tolist() == want.tolist()
        assert (teacher.last_drafted, teacher.last_accepted) == stats and stats[0] > 0
    # encoder_outputs alone: the assistant needs no input_features
    enc = torch.randn(1, gd.CFG_T.max_src, gd.CFG_T.d_model, generator=torch.Generator().manual_seed(3))
    a = teacher.generate(encoder_outputs=(enc,), assistant_model=causal, max_new_tokens=5, language="en")
    b = teacher.generate(encoder_outputs=(enc,), assistant_model=full, max_new_tokens=5, language="en")
    assert a.tolist() == b.tolist()


def test_causal_lm_assistant_of_another_width_raises():
    import dataclasses
    from distil_whisper_amd import WhisperForCausalLM
    from distil_whisper_amd.engine import WhisperDims
    ops = RefOps("cpu", lowp=torch.float32)
    fields = gd.generation_fields(multilingual=True, suppress=True, timestamps=False)
    teacher, _, _, cfg_s = _models(ops, 311, fields)
    d = WhisperDims.from_any(cfg_s)
    narrow = WhisperForCausalLM(dataclasses.replace(d, d_model=d.d_model // 2, heads=d.heads // 2), ops=ops, seed=1)
    with pytest.raises(ValueError, match="d_model"):
        teacher.generate(gd.features(312, 1), assistant_model=narrow, max_new_tokens=4, language="en")
