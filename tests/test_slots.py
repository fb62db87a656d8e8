"""Continuous batching on the CPU: the torch slot step (`decoding.slot_step_torch`) against the numpy restatement
(tests/slots_cases.py) on planted launches; the scheduler `decoding.SlotDecoder` over the torch restatement of the kernels
(oracle.ref_ops in fp32: no `slot_step`, no `decode_token_rows`, so the torch slot step and the per-kernel form of
`engine.decode_multi_rows`) against every window decoded by `GreedyDecoder` at the same batch size, where equality is exact;
`PseudoLabeller` / `LongFormTranscriber` with `continuous=True` against themselves without it; the public surface.

The model is tests/assist_rows_cases.planted_pair's target: window kinds 0 and 1 run to their budget, kind 2 takes EOS at the first
weak step, so the rows of one batch end at different lengths; every decision is a quarter of the best score away from turning."""
import numpy as np
import pytest
import torch

from distil_whisper_amd import decoding
from distil_whisper_amd.decoding import GreedyDecoder, SlotDecoder, slot_step_torch
from oracle import gen_golden_decode as gd
from oracle.ref_ops import RefOps
from tests import assist_rows_cases as arc
from tests import slots_cases as sc

SEQ = [50, 61, 72, 83, 94, 105, 116, 127, 138, 149]
WEAK = (2, 5, 8)
PROMPT = [gd.SOT, gd.LANG["<|en|>"], gd.TRANSCRIBE, gd.NOTIMESTAMPS]
ROW_TOKENS = [400, 410, gd.EOS]


# ---- the slot step ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ts", [False, True])
@pytest.mark.parametrize("V", [1030, 51865, 51866])
def test_torch_slot_step_matches_the_restatement(V, ts):
    c = sc.make_launch(V, ts)
    tokens = torch.from_numpy(c["tokens"]).clone()
    S = tokens.shape[0]
    length, plen, budget = (torch.from_numpy(c[k]).to(torch.int32) for k in ("length", "plen", "budget"))
    done = torch.from_numpy(c["done"]).clone()
    row_t, cur = torch.full((S,), -5, dtype=torch.int32), torch.full((S, 1), -5, dtype=torch.long)
    mask = lambda ids: decoding.token_mask(ids, V, "cpu", torch.uint8)
    slot_step_torch(torch.from_numpy(c["logits"]).float(), V, tokens, length, plen, budget, done, row_t, cur,
                    suppress=mask(c["suppress"]), begin_suppress=mask(c["begin_suppress"]), timestamp_rules=c["ts"], eos=c["eos"],
                    min_new=c["min_new"])
    sc.check_launch(c, tokens.numpy(), length.tolist(), done.tolist(), row_t.tolist(), cur.numpy())


# ---- the scheduler ------------------------------------------------------------------------------------------------------------
def planted_target(ops, seed=21, dtype=torch.float32, width=128):
    """width 128: the tiny model of the decode fixtures; 384: seeded weights at the narrowest width that has the token step's
    attention kernels with the projection inside (on the CPU statement, fp32 and bf16, every decision of either keeps 24 % of the
    best score from turning)."""
    from distil_whisper_amd import student_init as si
    from distil_whisper_amd.engine import WhisperDims
    from distil_whisper_amd.modeling import WhisperForConditionalGeneration
    cfg, sd = gd.CFG_T, None
    if width != 128:
        cfg = WhisperDims(width, width // 64, 4 * width, 1, 2, gd.CFG_T.vocab, 80, max_src=128, pad_token_id=gd.EOS,
                          decoder_start_token_id=gd.SOT)
        sd = {k: v.cpu() for k, v in si.random_state_dict(cfg, seed, "cpu").items()}
    sd, _, enc = arc.planted_pair(gd.weights(seed) if sd is None else sd, len(PROMPT), SEQ, WEAK, ROW_TOKENS, cfg.d_model, cfg.max_src,
                                  scale=4.0, head_gain=4.0)
    return WhisperForConditionalGeneration(cfg, ops=ops, state_dict=sd, dtype=dtype), enc


def make_windows(enc, n, max_src, vary=True):
    """n windows: the kind (encoder rows of planted row n % 3) decides where the row ends; prompt lengths and budgets vary."""
    out = []
    for i in range(n):
        kind = i % 3
        prompt = PROMPT + ([SEQ[0]] if vary and i % 4 == 1 else []) + ([SEQ[1], SEQ[0]] if vary and i % 4 == 3 else [])
        out.append((f"w{i}", enc[kind * max_src:(kind + 1) * max_src], prompt, (9, 7, 5)[i % 3] if vary else 9))
    return out


def greedy_rows(engine, windows, S, eos, count=None, **kw):
    """Every window decoded by GreedyDecoder at batch size S (the window in every row), cut behind its EOS."""
    out = {}
    for key, enc, prompt, max_new in windows:
        dec = GreedyDecoder(engine, S, len(prompt) + max_new, eos_token_id=eos, pad_token_id=eos, use_graphs=False, check_every=1, **kw)
        row = dec.run(enc.repeat(S, 1), torch.tensor([prompt] * S, device=enc.device), max_new)[0].tolist()
        out[key] = row[:row.index(eos, len(prompt)) + 1] if eos in row[len(prompt):] else row
    return out


def batch_path_steps(windows, S, eos, rows):
    """Token steps of the batch path over the same windows in plan order, S per batch: a batch runs until its longest row is done."""
    steps = 0
    for b0 in range(0, len(windows), S):
        steps += max(len(rows[w[0]]) for w in windows[b0:b0 + S]) - 1
    return steps


@pytest.mark.parametrize("n_windows,S,check_every", [(7, 3, 2), (7, 3, 8), (5, 2, 1), (1, 3, 4), (0, 3, 4), (4, 4, 3)])
def test_every_window_equals_that_window_decoded_by_the_batch_decoder(n_windows, S, check_every):
    ops = RefOps("cpu", lowp=torch.float32)
    assert not hasattr(ops, "slot_step") and not hasattr(ops, "decode_token_rows")
    model, enc = planted_target(ops)
    windows = make_windows(enc, n_windows, model.dims.max_src)
    dec = SlotDecoder(model.engine, S, len(PROMPT) + 2 + 9, gd.EOS, suppress_tokens=gd.SUPPRESS, check_every=check_every)
    got = [(k, r.tolist()) for k, r in dec.run(iter(windows))]
    want = greedy_rows(model.engine, windows, S, gd.EOS, suppress_tokens=gd.SUPPRESS)
    assert sorted(k for k, _ in got) == sorted(want) and len(got) == n_windows
    for k, row in got:
        assert row == want[k], k
    if n_windows == 0:
        assert dec.steps == 0
        return
    lens = sorted(len(r) for _, r in got)
    if n_windows >= 4:
        assert lens[0] < lens[-1], "every window ended at the same length"
        assert any(r[-1] == gd.EOS for _, r in got) and any(r[-1] != gd.EOS for _, r in got)
    # (a finished slot idles until the next look at the rows: with rows of a dozen tokens the count is held at check_every <= 2;
    # at 8 the seven windows take 40 steps against the batch path's 38)
    if n_windows > S and check_every <= 2:
        assert dec.steps < batch_path_steps(windows, S, gd.EOS, want), (dec.steps, lens)
    # the decoder is reusable: the same windows through the same buffers
    again = {k: r.tolist() for k, r in dec.run(iter(windows))}
    assert again == dict(got)


def test_slot_decoder_under_the_timestamp_rules_and_min_new_tokens():
    ops = RefOps("cpu", lowp=torch.float32)
    model, enc = planted_target(ops)
    prompt = PROMPT[:3]
    rules = dict(no_timestamps_token_id=gd.NOTIMESTAMPS, max_initial_timestamp_index=50)
    windows = [(i, enc[(i % 3) * model.dims.max_src:(i % 3 + 1) * model.dims.max_src], prompt, 8) for i in range(5)]
    for min_new in (0, 5):
        dec = SlotDecoder(model.engine, 2, len(prompt) + 8, gd.EOS, suppress_tokens=gd.SUPPRESS, timestamp_rules=rules,
                          min_new_tokens=min_new, check_every=3)
        got = dict((k, r.tolist()) for k, r in dec.run(windows))
        ref = GreedyDecoder(model.engine, 1, len(prompt) + 8, eos_token_id=gd.EOS, suppress_tokens=gd.SUPPRESS, use_graphs=False,
                            timestamp_rules=dict(rules, begin_index=len(prompt)), check_every=1)
        for k, e, p, m in windows:
            row = ref.run(e, torch.tensor([p]), m, min_new_tokens=min_new)[0].tolist()
            row = row[:row.index(gd.EOS, len(p)) + 1] if gd.EOS in row[len(p):] else row
            assert got[k] == row, (k, min_new)
            assert row[len(p)] > gd.NOTIMESTAMPS                          # the rules were on: the first token is a timestamp
            assert min_new == 0 or len(row) - len(p) > min_new or row[-1] != gd.EOS


def test_slot_decoder_refuses_what_it_cannot_hold():
    ops = RefOps("cpu", lowp=torch.float32)
    model, enc = planted_target(ops)
    with pytest.raises(ValueError, match="eos_token_id"):
        SlotDecoder(model.engine, 2, 12, None)
    with pytest.raises(ValueError, match="max_target_positions"):
        SlotDecoder(model.engine, 2, model.dims.max_tgt + 1, gd.EOS)
    dec = SlotDecoder(model.engine, 2, 12, gd.EOS)
    for prompt, max_new in ((PROMPT, 9), ([], 3), (PROMPT, 0)):
        with pytest.raises(ValueError, match="max_len"):
            list(dec.run([("k", enc[:model.dims.max_src], prompt, max_new)]))


# ---- PseudoLabeller / LongFormTranscriber -------------------------------------------------------------------------------------
def _micro():
    from distil_whisper_amd.modeling import WhisperFeatureExtractor, WhisperForConditionalGeneration
    from oracle import whisper_oracle as wo
    cfg = wo.OracleConfig(128, 2, 256, 2, 2, 1000, 80, pad_token_id=900, decoder_start_token_id=901)
    ops = RefOps("cpu", lowp=torch.float32)
    model = WhisperForConditionalGeneration(cfg, ops=ops, state_dict=wo.init_state_dict(cfg, 23, std=0.1))
    return cfg, model, WhisperFeatureExtractor(feature_size=80, ops=ops)


def count_steps(monkeypatch):
    n = {"batch": 0}
    step = GreedyDecoder._run_step

    def spy(self, *a, **k):
        n["batch"] += 1
        return step(self, *a, **k)
    monkeypatch.setattr(GreedyDecoder, "_run_step", spy)
    return n


def test_pseudo_labeller_continuous_gives_the_same_labels(monkeypatch):
    from distil_whisper_amd.pseudo_label import PseudoLabeller
    cfg, model, fe = _micro()
    rng = np.random.default_rng(10)
    audios = [0.1 * rng.standard_normal(n).astype(np.float32) for n in (200_000, 150_000, 300_000, 100_000, 260_000, 90_000, 120_000)]
    spk = [0, 0, 0, 1, 2, 3, 4]
    plain = PseudoLabeller(model, fe, batch_size=2, max_new_tokens=10, eos_token_id=905, use_graphs=False)
    ref = plain(audios, spk)
    # an EOS that some packs emit early and others never: the labels end at different lengths
    firsts = sorted({t for row in ref[0] for t in row[2:6]})
    eos = firsts[len(firsts) // 2]
    kw = dict(batch_size=2, max_new_tokens=10, eos_token_id=eos, use_graphs=False, suppress_tokens=[3, 4], begin_suppress_tokens=[eos])
    n = count_steps(monkeypatch)
    want = PseudoLabeller(model, fe, **kw)(audios, spk)
    lab = PseudoLabeller(model, fe, continuous=True, check_every=2, **kw)
    got = lab(audios, spk)
    assert got == want and len(want[1]) == 6
    assert len({len(r) for r in want[0]}) > 1
    assert 0 < lab.slot_decoder.steps < n["batch"]
    assert lab(audios[:0], spk[:0]) == ([], [], [])


@pytest.mark.parametrize("timestamps", [False, True])
def test_transcriber_continuous_gives_the_same_transcripts(timestamps):
    from distil_whisper_amd.longform import LongFormTranscriber
    cfg, model, fe = _micro()
    rng = np.random.default_rng(6)
    audios = [0.1 * rng.standard_normal(n).astype(np.float32) for n in (1_100_000, 480_000, 700_000)]
    kw = dict(batch_size=2, chunk_length_s=30.0, max_new_tokens=12, prompt_ids=[901], eos_token_id=902,
              suppress_tokens=list(range(903, 912)), use_graphs=False)
    if timestamps:
        kw.update(return_timestamps=True, no_timestamps_token_id=912)
    want = LongFormTranscriber(model, fe, **kw)(audios)
    tr = LongFormTranscriber(model, fe, continuous=True, check_every=3, **kw)
    assert tr(audios) == want and len(want) == 3 and any(want)
    assert tr.slot_decoder.steps > 0


def test_continuous_refusals_come_before_the_encoder_runs(monkeypatch):
    from distil_whisper_amd.longform import LongFormTranscriber
    from distil_whisper_amd.pseudo_label import PseudoLabeller
    cfg, model, fe = _micro()

    def no_encode(*a, **k):
        raise AssertionError("the encoder ran before the refusal")
    monkeypatch.setattr(type(model.engine), "encode", no_encode)
    kw = dict(batch_size=2, max_new_tokens=4, eos_token_id=902, continuous=True)
    for extra in (dict(num_beams=2), dict(assistant_model=model),
                  dict(timestamp_rules=dict(no_timestamps_token_id=912, max_initial_timestamp_index=50)), dict(repetition_penalty=1.2),
                  dict(no_repeat_ngram_size=3), dict(sequence_bias={(50,): 1.0}), dict(bad_words_ids=[[50]])):
        with pytest.raises(NotImplementedError):
            PseudoLabeller(model, fe, **kw, **extra)
    with pytest.raises(ValueError, match="overlap"):
        PseudoLabeller(model, fe, overlap=True, **kw)
    for extra in (dict(repetition_penalty=1.2), dict(no_repeat_ngram_size=3), dict(sequence_bias={(50,): 1.0}), dict(bad_words_ids=[[50]])):
        with pytest.raises(NotImplementedError, match="continuous"):
            LongFormTranscriber(model, fe, **kw, **extra)
    with pytest.raises(ValueError, match="overlap"):
        LongFormTranscriber(model, fe, overlap=True, **kw)
    with pytest.raises(ValueError, match="eos_token_id"):
        PseudoLabeller(model, fe, batch_size=2, max_new_tokens=4, continuous=True)
    assert PseudoLabeller(model, fe, batch_size=2, max_new_tokens=4, eos_token_id=902).continuous is False


def test_the_entries_are_declared_and_bound():
    import os
    from distil_whisper_amd import build, ops_hip
    header = open(os.path.join(os.path.dirname(os.path.abspath(ops_hip.__file__)), "..", "include", "dwamd.h")).read()
    for name in ("dw_decode_attn_proj_rows", "dw_decode_token_rows", "dw_slot_step"):
        assert f"int {name}(" in header and name in ops_hip.EXPORTED_SYMBOLS
    assert "slots.hip" in build.SOURCES
    for method in ("decode_attn_proj_rows", "decode_token_rows", "slot_step"):
        assert hasattr(ops_hip.HipOps, method)
