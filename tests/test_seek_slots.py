"""The timestamp seek loop on slots, on the CPU (oracle.ref_ops in fp32: the torch slot step and the per-kernel token step).

* `decoding.slot_step_torch` with the two window scores (`dw_slot_step_scores` is the kernel) against their float64 restatement
  (tests/seek_slots_cases.scores_launch) on the planted launches of tests/slots_cases.py.
* `SlotDecoder.WAIT`.
* `seek_decode(slots=N)` against `seek_decode()` on a planted model (tests/seek_slots_cases.py) whose utterances need 1, 2 and 3
  windows, segment for segment, with spies on the encoder and the schedule.
* The thresholds: skips and segments of both loops agree, and the slot loop runs no teacher-forced pass.
* `generate(seek_slots=)` on the seeded scenarios of test_timestamp_seek_loop_matches_transformers_live, `PseudoLabeller(seek_slots=
  True)`, every refusal with the encoder made to fail, the public surface."""
import numpy as np
import pytest
import torch

from distil_whisper_amd import decoding
from distil_whisper_amd.decoding import GreedyDecoder, SlotDecoder, slot_step_torch
from oracle import gen_golden_decode as gd
from oracle.ref_ops import RefOps
from tests import seek_slots_cases as ss
from tests import slots_cases as sc
from tests.test_slots import PROMPT, _micro, make_windows, planted_target

REORDER = 2.0                                   # this project's allowance for the same fp32 reductions in another order


# ---- the slot step with scores ------------------------------------------------------------------------------------------------
def torch_state(c, dev="cpu"):
    S = c["tokens"].shape[0]
    t = dict(tokens=torch.from_numpy(c["tokens"]).clone().to(dev),
             done=torch.from_numpy(np.asarray(c["done"], dtype=bool)).clone().to(dev),
             row_t=torch.full((S,), -5, dtype=torch.int32, device=dev), cur=torch.full((S, 1), -5, dtype=torch.long, device=dev))
    for k in ("length", "plen", "budget"):
        t[k] = torch.from_numpy(np.asarray(c[k])).to(torch.int32).to(dev)
    return t


def score_buffers(c, dev="cpu"):
    return (torch.from_numpy(c["lp0"]).float().to(dev), torch.from_numpy(c["nsp0"]).float().to(dev),
            torch.from_numpy(c["nsp_pos"]).to(torch.int32).to(dev))


def check_state(c, t):
    w_tok, w_len, w_done, w_rt, w_cur, _ = c["want"]
    assert t["tokens"].cpu().numpy().tolist() == w_tok.tolist()
    assert t["length"].tolist() == w_len.tolist() and t["done"].tolist() == w_done.tolist()
    assert t["row_t"].tolist() == w_rt.tolist() and t["cur"].view(-1).tolist() == w_cur.tolist()


def deviations(c, lp, nsp):
    """Largest |lp - float64| over the generated slots and |nsp - float64| over all; untouched entries must be untouched."""
    lp, nsp = np.asarray(lp, dtype=np.float64), np.asarray(nsp, dtype=np.float64)
    for i in range(len(lp)):
        if i not in c["gen"]:
            assert lp[i] == c["lp0"][i], c["names"][i]
        if c["nsp"][i] == c["nsp0"][i]:
            assert nsp[i] == c["nsp0"][i], c["names"][i]
    gen = c["gen"]
    return float(np.max(np.abs(lp[gen] - c["lp"][gen]))), float(np.max(np.abs(nsp - c["nsp"])))


def nsp_column(c, on=True):
    if not on:
        return -1
    if c["ts"] is not None:
        return c["ts"]["no_timestamps_token_id"] - 1
    taken = set(c["suppress"]) | set(c["begin_suppress"]) | {c["eos"]} | set(np.asarray(c["want"][0]).reshape(-1).tolist())
    return next(col for col in range(5, 200) if col not in taken)   # a column the rules leave alone and no slot picks


@pytest.mark.parametrize("ts", [False, True])
@pytest.mark.parametrize("V", [1030, 51865, 51866])
def test_torch_slot_step_scores_against_float64(V, ts):
    base = sc.make_launch(V, ts)
    mask = lambda ids: decoding.token_mask(ids, V, "cpu", torch.uint8)
    logits = None
    for on in (True, False):
        c = ss.scores_launch(base, nsp_column(base, on))
        logits = torch.from_numpy(c["logits"]).float()
        kw = dict(suppress=mask(c["suppress"]), begin_suppress=mask(c["begin_suppress"]), timestamp_rules=c["ts"], eos=c["eos"],
                  min_new=c["min_new"])
        t = torch_state(c)
        lp, nsp, pos = score_buffers(c)
        slot_step_torch(logits, V, t["tokens"], t["length"], t["plen"], t["budget"], t["done"], t["row_t"], t["cur"], lp_sum=lp, nsp=nsp,
                        nsp_pos=pos, nsp_col=nsp_column(base, on), **kw)
        check_state(c, t)
        plain = torch_state(c)                     # the plain step: the same tokens and state
        slot_step_torch(logits, V, plain["tokens"], plain["length"], plain["plen"], plain["budget"], plain["done"], plain["row_t"],
                        plain["cur"], **kw)
        check_state(c, plain)
        d_lp, d_nsp = deviations(c, lp.numpy(), nsp.numpy())
        # the bound: processed_scores + log_softmax in fp32 on the same rows, against the same float64 numbers
        ref = []
        for i in c["gen"]:
            n, P = int(c["length"][i]), int(c["plen"][i])
            s = decoding.processed_scores(logits[i:i + 1], torch.from_numpy(c["tokens"][i:i + 1]), n, begin_index=P, eos=c["eos"],
                                          no_eos=n - P < c["min_new"], first=n == P, suppress=kw["suppress"],
                                          begin_suppress=kw["begin_suppress"], timestamp_rules=c["ts"])
            got = float(torch.log_softmax(s[0], -1)[int(c["want"][0][i, n])])
            ref.append(abs(np.float64(np.float32(c["lp0"][i]) + np.float32(got)) - c["lp"][i]))
        print(f"V {V} ts {ts} nsp_col {nsp_column(base, on)}: lp deviation {d_lp:.3e} (fp32 log_softmax {max(ref):.3e}), nsp {d_nsp:.3e}")
        assert d_lp <= REORDER * max(ref) and d_nsp <= REORDER * max(ref)


# ---- WAIT -----------------------------------------------------------------------------------------------------------------------
def test_a_source_may_answer_wait_and_a_plain_iterator_behaves_as_before():
    ops = RefOps("cpu", lowp=torch.float32)
    model, enc = planted_target(ops)
    windows = make_windows(enc, 7, model.dims.max_src)
    dec = SlotDecoder(model.engine, 3, len(PROMPT) + 2 + 9, gd.EOS, suppress_tokens=gd.SUPPRESS, check_every=2)
    want = {k: r.tolist() for k, r in dec.run(iter(windows))}
    steps = dec.steps
    assert len(want) == 7

    live, asked = [0], [0]

    def source():
        """Hands out a window only while fewer than two are live, else WAIT: rows are live whenever it says so."""
        todo = list(windows)
        while todo:
            asked[0] += 1
            if live[0] >= 2:
                yield SlotDecoder.WAIT
                continue
            live[0] += 1
            yield todo.pop(0)
    got = {}
    for k, r in dec.run(source()):
        live[0] -= 1
        got[k] = r.tolist()
    assert got == want and asked[0] > 7 and dec.steps > steps
    # a source that waits although no row is live can never be served: loud, not a hang
    with pytest.raises(RuntimeError, match="WAIT"):
        list(dec.run(iter([SlotDecoder.WAIT])))
    assert {k: r.tolist() for k, r in dec.run(iter(windows))} == want


# ---- the scheduler --------------------------------------------------------------------------------------------------------------
def count_steps(monkeypatch):
    n = {"batch": 0}
    step = GreedyDecoder._run_step

    def spy(self, *a, **k):
        n["batch"] += 1
        return step(self, *a, **k)
    monkeypatch.setattr(GreedyDecoder, "_run_step", spy)
    return n


def seek_args(feats, max_frames, init):
    return (feats, max_frames, init, lambda P: (ss.MAX_NEW, 0), gd.EOS, gd.EOS, gd.NOTIMESTAMPS, 50)


def lockstep_conditions(spy, B, expected_windows):
    """What the scenario was built for, asserted on the lockstep loop's own run."""
    counts = [len(w) for w in spy.windows_of(B)]
    assert counts == expected_windows[:B]
    passes = spy.passes()
    ends = [(s[-1] >= ss.TB, len(s) > 1 and s[-2] >= ss.TB) for p in passes for s in p]
    conditions = dict(one_window=1 in counts, three_windows=max(counts) >= 3,
                      lengths_differ_in_a_pass=any(len({len(s) for s in p}) > 1 for p in passes),
                      single_ending=(True, False) in ends, closed_pair=(True, True) in ends)
    return conditions


@pytest.mark.parametrize("n_utt,N,check_every,prompt,multilingual", [
    (7, 1, 8, False, False), (7, 2, 1, False, False), (7, 3, 3, False, False), (7, 3, 2, True, False), (2, 3, 8, False, False),
    (4, 2, 2, False, True), (7, 3, 8, False, True)])
def test_slot_schedule_equals_the_lockstep_loop(monkeypatch, n_utt, N, check_every, prompt, multilingual):
    ops = RefOps("cpu", lowp=torch.float32)
    prompt_ids = [gd.STARTOFPREV, 41, 42] if prompt else None
    P = len(ss.INIT) + (3 if prompt else 0)
    model, enc = ss.planted_seek_model(ops, P)
    W = 2 * model.dims.max_src
    feats, max_frames, expected = ss.utterances(W, n_utt)
    B = feats.shape[0]
    langs = list(gd.LANG.values())
    init = [[gd.SOT, langs[b % len(langs)] if multilingual else gd.LANG["<|en|>"], gd.TRANSCRIBE] for b in range(B)]
    kw = dict(suppress_tokens=gd.SUPPRESS, prompt_ids=prompt_ids)
    spy = ss.Spy(monkeypatch, model, enc)
    n = count_steps(monkeypatch)
    want = model.seek_decode(*seek_args(feats, max_frames, init), **kw)
    cond = lockstep_conditions(spy, B, expected)
    if n_utt == 7:
        assert all(cond.values()), cond
    else:
        assert cond["three_windows"] or cond["closed_pair"], cond
    lock_windows, lock_steps = spy.windows_of(B), n["batch"]
    assert ("decode",) not in spy.log
    spy.clear()
    margins = ss.margin_spy(monkeypatch)
    got = model.seek_decode(*seek_args(feats, max_frames, init), slots=N, check_every=check_every, **kw)
    assert min(margins) >= ss.MIN_KEEP, min(margins)
    ss.same_segments(got, want)
    assert any(len(r) > 1 for r in got) and all(got)
    assert spy.windows_of(B) == lock_windows                       # the same windows, utterance by utterance, in order
    held = spy.check_schedule(B, N)
    st = model.last_seek_stats
    assert st["max_held"] == held and st["windows"] == sum(expected[:B]) and st["encoder_batches"] == spy.encoder_batches()
    assert n["batch"] == lock_steps                                # no lockstep pass ran
    print(f"utterances {B}, slots {N}, check_every {check_every}: {st['steps']} slot steps against {lock_steps} lockstep steps, "
          f"encoder calls {st['encoder_batches']}, most windows held {held}")
    # a second call on the same model reuses the decoder and its buffers
    dec = [d for k, d in model._seek_slot_decoders.items()]
    assert len(dec) == 1
    spy.clear()
    ss.same_segments(model.seek_decode(*seek_args(feats, max_frames, init), slots=N, check_every=check_every, **kw), want)
    assert [d for k, d in model._seek_slot_decoders.items()] == dec and dec[0].steps == 2 * st["steps"]
    if B > N and check_every <= 2:
        # a token step of N rows against a token step of N rows: the lockstep loop over batches of N utterances, which is how
        # the labeller feeds it (one call over all B utterances steps B rows at a time)
        before = n["batch"]
        for b0 in range(0, B, N):
            model.seek_decode(*seek_args(feats[b0:b0 + N], max_frames[b0:b0 + N], init[b0:b0 + N]), **kw)
        assert st["steps"] < n["batch"] - before, (st["steps"], n["batch"] - before)
        print(f"  the lockstep loop over batches of {N}: {n['batch'] - before} steps")


def test_slot_schedule_refuses_prompts_of_different_lengths():
    ops = RefOps("cpu", lowp=torch.float32)
    model, enc = ss.planted_seek_model(ops, 3)
    feats, max_frames, _ = ss.utterances(2 * model.dims.max_src, 2)
    with pytest.raises(NotImplementedError, match="one length"):
        model.seek_decode(*seek_args(feats, max_frames, [ss.INIT, ss.INIT + [gd.NOTIMESTAMPS]]), slots=2)
    with pytest.raises(ValueError, match="slots"):
        model.seek_decode(*seek_args(feats, max_frames, [ss.INIT] * 2), slots=0)
    with pytest.raises(ValueError, match="slots"):
        model.seek_decode(*seek_args(feats, max_frames, [ss.INIT] * 2), cross_kv_dtype="fp8")


# ---- the thresholds -------------------------------------------------------------------------------------------------------------
def widest_gap(values):
    v = sorted(set(values))
    assert len(v) >= 2
    w, i = max((b - a, i) for i, (a, b) in enumerate(zip(v, v[1:])))
    return (v[i] + v[i + 1]) / 2, w


def thresholds_from_lockstep(model, args, kw):
    """Each window's (average log-probability, no-speech probability) as the lockstep loop's `scores_of` computes them (thresholds
    that decide nothing), and the two thresholds in the middle of the widest gaps."""
    model.seek_decode(*args, logprob_threshold=-1e9, no_speech_threshold=2.0, **kw)
    scores = list(model.last_window_scores)
    lp_thr, lp_gap = widest_gap([s[2] for s in scores])
    ns_thr, ns_gap = widest_gap([s[3] for s in scores])
    return scores, (lp_thr, lp_gap), (ns_thr, ns_gap)


def test_thresholds_are_judged_on_the_slot_steps_own_numbers(monkeypatch):
    ops = RefOps("cpu", lowp=torch.float32)
    model, enc = ss.planted_seek_model(ops, 3)
    feats, max_frames, _ = ss.utterances(2 * model.dims.max_src)
    B = feats.shape[0]
    args, kw = seek_args(feats, max_frames, [ss.INIT] * B), dict(suppress_tokens=gd.SUPPRESS)
    spy = ss.Spy(monkeypatch, model, enc)
    scores, (lp_thr, lp_gap), (ns_thr, ns_gap) = thresholds_from_lockstep(model, args, kw)
    # the same windows in the bf16 statement: what the lockstep numbers themselves move by
    low, enc_low = ss.planted_seek_model(RefOps("cpu", lowp=torch.bfloat16), 3, dtype=torch.bfloat16)
    ss.Spy(monkeypatch, low, enc_low)
    low.seek_decode(*args, logprob_threshold=-1e9, no_speech_threshold=2.0, **kw)
    assert [s[:2] for s in low.last_window_scores] == [s[:2] for s in scores]
    dev_lp = max(abs(a[2] - b[2]) for a, b in zip(low.last_window_scores, scores))
    dev_ns = max(abs(a[3] - b[3]) for a, b in zip(low.last_window_scores, scores))
    print(f"logprob gap {lp_gap:.4f} (bf16 deviation {dev_lp:.2e}), no-speech gap {ns_gap:.3e} (bf16 deviation {dev_ns:.2e})")
    assert lp_gap > 4 * dev_lp and ns_gap > 4 * dev_ns
    th = dict(logprob_threshold=lp_thr, no_speech_threshold=ns_thr)
    spy.clear()
    want = model.seek_decode(*args, **th, **kw)
    lock = list(model.last_window_scores)
    assert ("decode",) in spy.log                                  # the lockstep loop's teacher-forced pass
    skipped = [s for s in lock if s[2] < lp_thr and s[3] > ns_thr]
    assert skipped and len(skipped) < len(lock)
    for N in (2, 3):
        spy.clear()
        got = model.seek_decode(*args, slots=N, check_every=2, **th, **kw)
        assert ("decode",) not in spy.log                          # no rescoring pass
        ss.same_segments(got, want)
        mine = sorted(model.last_window_scores)
        assert [s[:2] for s in mine] == [s[:2] for s in sorted(lock)]
        assert [(s[2] < lp_thr, s[3] > ns_thr) for s in mine] == [(s[2] < lp_thr, s[3] > ns_thr) for s in sorted(lock)]
        for a, b in zip(mine, sorted(lock)):
            assert abs(a[2] - b[2]) < 1e-5 and abs(a[3] - b[3]) < 1e-8
        spy.check_schedule(B, N)
    with pytest.raises(ValueError, match="logprob_threshold"):
        model.seek_decode(*args, slots=2, no_speech_threshold=0.5, **kw)


# ---- generate / PseudoLabeller ----------------------------------------------------------------------------------------------------
def seeded_scenarios(seed):
    long1 = torch.cat([gd.features(seed + 1, 1), gd.features(seed + 2, 1), gd.features(seed + 3, 1)[..., :1500]], -1)
    a = torch.cat([gd.features(seed + 4, 1), gd.features(seed + 5, 1)], -1)
    b = torch.cat([gd.features(seed + 6, 1)[..., :2000], torch.zeros(1, 80, 4000)], -1)
    mask = torch.ones(2, 6000, dtype=torch.long)
    mask[1, 2000:] = 0
    return ((gd.features(seed + 1, 2), dict(max_new_tokens=6, return_timestamps=True, language="en")),
            (long1, dict(max_new_tokens=5, return_timestamps=True, language="de")),
            (torch.cat([a, b], 0), dict(max_new_tokens=4, return_timestamps=True, language="en", attention_mask=mask)))


def test_generate_with_seek_slots_equals_generate():
    """The scenarios of test_timestamp_seek_loop_matches_transformers_live, which holds `generate()` to `transformers`: every
    utterance is compared, none is left out."""
    from tests.test_decode_parity import _model
    ops = RefOps("cpu", lowp=torch.float32)
    fields = gd.generation_fields(multilingual=True, suppress=True, timestamps=True)
    multi = 0
    for seed in (300, 301):
        model = _model(ops, gd.CFG_T, gd.weights(seed), fields)
        for i, (feats, kw) in enumerate(seeded_scenarios(seed)):
            want = model.generate(feats, return_segments=True, **kw)
            got = model.generate(feats, return_segments=True, seek_slots=2, **kw)
            assert got["sequences"].tolist() == want["sequences"].tolist(), (seed, i)
            ss.same_segments(got["segments"], want["segments"])
            multi += max(len(s) for s in want["segments"]) > 1
            if seed != 300:
                continue
            assert model.generate(feats, seek_slots=3, temperature=0.0, **kw).tolist() == model.generate(feats, **kw).tolist()
            out = model.generate(feats, seek_slots=1, return_dict_in_generate=True, **kw)
            assert out.sequences.tolist() == want["sequences"].tolist() and len(out.segments) == feats.shape[0]
            pid = torch.tensor([fields["prev_sot_token_id"], 31, 32, 33])
            assert model.generate(feats, prompt_ids=pid, seek_slots=2, **kw).tolist() == model.generate(feats, prompt_ids=pid, **kw).tolist()
            th = dict(logprob_threshold=-1.0, no_speech_threshold=0.6, compression_ratio_threshold=1.35, temperature=0.0)
            assert model.generate(feats, seek_slots=2, **th, **kw).tolist() == model.generate(feats, **th, **kw).tolist()
        # language detection runs before the slots start
        feats, kw = seeded_scenarios(seed)[0]
        kw = {k: v for k, v in kw.items() if k != "language"}
        assert model.generate(feats, seek_slots=2, **kw).tolist() == model.generate(feats, **kw).tolist()
    assert multi >= 4


def labeller_inputs():
    rng = np.random.default_rng(10)
    audios = [0.1 * rng.standard_normal(n).astype(np.float32) for n in (200_000, 150_000, 300_000, 100_000, 260_000, 90_000, 120_000)]
    return audios, [0, 0, 0, 1, 2, 3, 4]


def test_pseudo_labeller_with_seek_slots_gives_the_same_labels():
    from distil_whisper_amd.pseudo_label import PseudoLabeller
    cfg, model, fe = _micro()
    audios, spk = labeller_inputs()
    rules = dict(no_timestamps_token_id=912, max_initial_timestamp_index=50)
    kw = dict(batch_size=2, max_new_tokens=10, eos_token_id=905, use_graphs=False, suppress_tokens=[3, 4], timestamp_rules=rules,
              prompt_ids=[901, 902, 903])
    want = PseudoLabeller(model, fe, **kw)(audios, spk)
    assert len(want[1]) == 6 and any(want[0])
    for group in (1, 2, 8):                                        # 6 packs on 2 slots: groups of 2, 4 and all
        lab = PseudoLabeller(model, fe, seek_slots=True, check_every=2, seek_group=group, **kw)
        assert lab(audios, spk) == want, group
        assert model.last_seek_stats["steps"] > 0 and max(model.last_seek_stats["encoder_batches"]) <= 2
    assert lab(audios[:0], spk[:0]) == ([], [], [])


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_every_refusal_comes_before_the_encoder_runs(monkeypatch):
    from distil_whisper_amd.pseudo_label import PseudoLabeller
    from tests.test_decode_parity import _model
    ops = RefOps("cpu", lowp=torch.float32)
    fields = gd.generation_fields(multilingual=True, suppress=True, timestamps=True)
    model = _model(ops, gd.CFG_T, gd.weights(300), fields)

    def no_encode(*a, **k):
        raise AssertionError("the encoder ran before the refusal")
    monkeypatch.setattr(type(model.engine), "encode", no_encode)
    feats = gd.features(1, 2)
    base = dict(return_timestamps=True, language="en", max_new_tokens=4, seek_slots=2)
    for extra in (dict(temperature=0.4), dict(temperature=(0.0, 0.4), logprob_threshold=-1.0), dict(condition_on_prev_tokens=True),
                  dict(num_beams=2), dict(assistant_model=model), dict(return_token_timestamps=True), dict(repetition_penalty=1.2),
                  dict(no_repeat_ngram_size=3), dict(sequence_bias={(50,): 1.0}), dict(bad_words_ids=[[50]]), dict(use_cache=False),
                  dict(output_scores=True, return_dict_in_generate=True), dict(output_logits=True, return_dict_in_generate=True),
                  dict(decoder_input_ids=torch.tensor([[gd.SOT]] * 2))):
        with pytest.raises(NotImplementedError, match="seek_slots"):
            model.generate(feats, **base, **extra)
    for kw in (dict(base, return_timestamps=False), dict(base, seek_slots=0), dict(base, seek_slots=-3),
               dict(base, force_unique_generate_call=True)):
        with pytest.raises(ValueError, match="seek_slots"):
            model.generate(feats, **kw)
    # (the FP8 cache inside the seek loop without slots keeps raising: tests/test_cross_kv_fp8.py, at a width that has the kernel)
    # seek_decode itself
    args = seek_args(feats, [3000, 3000], [ss.INIT] * 2)
    for extra in (dict(temperatures=(0.0, 0.2)), dict(condition_on_prev_tokens=True), dict(num_beams=2), dict(assistant=(model.engine, None)),
                  dict(token_timestamps=dict(alignment_heads=[[0, 0]], num_frames=None, time_precision=0.02)),
                  dict(repetition_penalty=1.3), dict(no_repeat_ngram_size=2)):
        with pytest.raises(NotImplementedError, match="slots"):
            model.seek_decode(*args, slots=2, **extra)
    # the labeller
    cfg, micro, fe = _micro()
    monkeypatch.setattr(type(micro.engine), "encode", no_encode)
    rules = dict(no_timestamps_token_id=912, max_initial_timestamp_index=50)
    kw = dict(batch_size=2, max_new_tokens=4, eos_token_id=902, seek_slots=True)
    for extra in (dict(num_beams=2), dict(assistant_model=micro), dict(repetition_penalty=1.2), dict(no_repeat_ngram_size=3),
                  dict(sequence_bias={(50,): 1.0}), dict(bad_words_ids=[[50]])):
        with pytest.raises(NotImplementedError):
            PseudoLabeller(micro, fe, timestamp_rules=rules, **kw, **extra)
    with pytest.raises(ValueError, match="timestamp_rules"):
        PseudoLabeller(micro, fe, **kw)
    with pytest.raises(ValueError, match="overlap"):
        PseudoLabeller(micro, fe, timestamp_rules=rules, overlap=True, **kw)
    with pytest.raises(ValueError, match="seek_group"):
        PseudoLabeller(micro, fe, timestamp_rules=rules, seek_group=0, **kw)
    # unchanged: continuous batching refuses the seek loop
    with pytest.raises(NotImplementedError):
        PseudoLabeller(micro, fe, batch_size=2, max_new_tokens=4, eos_token_id=902, continuous=True, timestamp_rules=rules)


def test_the_scores_entry_is_declared_and_bound():
    import inspect
    import os
    from distil_whisper_amd import ops_hip
    root = os.path.join(os.path.dirname(os.path.abspath(ops_hip.__file__)), "..")
    header = open(os.path.join(root, "include", "dwamd.h")).read()
    assert "int dw_slot_step_scores(" in header and "dw_slot_step_scores" in ops_hip.EXPORTED_SYMBOLS
    assert "`dw_slot_step_scores`" in open(os.path.join(root, "INTEGRATION.md")).read()
    assert {"lp_sum", "nsp", "nsp_pos", "nsp_col"} <= set(inspect.signature(ops_hip.HipOps.slot_step).parameters)
    assert SlotDecoder.WAIT is not None and "scores" in inspect.signature(SlotDecoder.__init__).parameters
