"""The timestamp seek loop on slots, on the MI355X.

* `dw_slot_step_scores` on the planted launches of tests/slots_cases.py extended by tests/seek_slots_cases.scores_launch: every
  integer of the state exact and equal to the plain entry's; the log-probability sum and the no-speech probability against their
  float64 restatement, held to twice the largest deviation of `dw_score_tokens`' `logprob` on the same rows (the same fp32
  reductions in another order); eight consecutive steps on one slot within eight times the one-step bound; refusals write nothing.
* `seek_decode(slots=N)` against the lockstep loop on the planted model of tests/seek_slots_cases.py in bf16, at width 128 and 384,
  under `dw_debug_set` key 7 = 0 and the default, graphs against eager, replayed over the same buffers; an utterance whose lockstep
  decode met a margin within EXACT_ULPS bf16 ulps is not held to equality (tests/test_slots_gpu.py).
* `cross_kv_dtype="fp8"` on slots against the bf16 slots; the thresholds judged on the slot step's numbers."""
import numpy as np
import pytest
import torch

from oracle import gen_golden_decode as gd
from tests import seek_slots_cases as ss
from tests import slots_cases as sc
from tests.test_assist_rows import EXACT_ULPS
from tests.test_seek_slots import (REORDER, check_state, deviations, nsp_column, score_buffers, seek_args, thresholds_from_lockstep,
                                   torch_state)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL = -1
KEY7_DEFAULT = 4


@pytest.fixture(scope="module")
def ops():
    from distil_whisper_amd.ops_hip import HipOps
    return HipOps(DEV)


@pytest.fixture()
def key7(ops):
    def set_key(value):
        assert ops.lib.dw_debug_set(7, value) == 0
    yield set_key
    ops.lib.dw_debug_set(7, KEY7_DEFAULT)


def rule_args(c, V):
    from distil_whisper_amd.decoding import token_mask
    r = c["ts"]
    return dict(suppress=token_mask(c["suppress"], V, DEV, torch.uint8), begin_suppress=token_mask(c["begin_suppress"], V, DEV, torch.uint8),
                ts_begin=-1 if r is None else r["no_timestamps_token_id"] + 1, max_initial=-1 if r is None else r["max_initial_timestamp_index"],
                eos=c["eos"], min_new=c["min_new"])


def padded_logits(rows, V, ld):
    lg = torch.full((rows.shape[0], ld), 50.0, dtype=torch.bfloat16, device=DEV)                # (a pad column would win if read)
    lg[:, :V] = torch.from_numpy(rows).to(DEV).bfloat16()
    return lg


# ---- dw_slot_step_scores --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ts", [False, True])
@pytest.mark.parametrize("V,ld", [(1030, 1032), (51865, 51872), (51866, 51868)])
def test_slot_step_scores_kernel_against_float64(ops, V, ld, ts):
    base = sc.make_launch(V, ts)
    for on in (True, False):
        col = nsp_column(base, on)
        c = ss.scores_launch(base, col)
        lg, kw = padded_logits(c["logits"], V, ld), rule_args(c, V)
        t = torch_state(c, DEV)
        lp, nsp, pos = score_buffers(c, DEV)
        ops.slot_step(lg, V, t["tokens"], t["length"], t["plen"], t["budget"], t["done"], t["row_t"], t["cur"], lp_sum=lp, nsp=nsp,
                      nsp_pos=pos, nsp_col=col, **kw)
        plain = torch_state(c, DEV)
        ops.slot_step(lg, V, plain["tokens"], plain["length"], plain["plen"], plain["budget"], plain["done"], plain["row_t"], plain["cur"], **kw)
        torch.cuda.synchronize()
        check_state(c, t)
        check_state(c, plain)
        for k in t:
            assert torch.equal(t[k], plain[k]), k
        d_lp, d_nsp = deviations(c, lp.cpu().numpy(), nsp.cpu().numpy())
        # dw_score_tokens on the same rows: slot i stands at step n - P of a row whose prompt has P tokens
        ref = []
        for i in c["gen"]:
            n, P = int(c["length"][i]), int(c["plen"][i])
            L = n - P + 1
            buf = torch.zeros((L, ld), dtype=torch.bfloat16, device=DEV)
            buf[L - 1] = lg[i]
            toks = torch.from_numpy(c["want"][0][i:i + 1]).to(DEV)
            _, _, logprob = ops.score_tokens(buf, V, toks, P, L, want_scores=False, **kw)
            one = np.float32(logprob[0, L - 1].item())
            ref.append(abs(np.float64(np.float32(c["lp0"][i]) + one) - c["lp"][i]))
        print(f"V {V} ld {ld} ts {ts} nsp_col {col}: lp deviation {d_lp:.3e}, dw_score_tokens {max(ref):.3e}, "
              f"ratio {d_lp / max(ref):.2f}; nsp deviation {d_nsp:.3e}")
        assert d_lp <= REORDER * max(ref) and d_nsp <= REORDER * max(ref)


def test_eight_steps_on_one_slot_add_up(ops):
    V, ld, P, steps, eos = 1030, 1032, 3, 8, 900
    rng = np.random.default_rng(8)
    rows = torch.from_numpy(2.0 * rng.standard_normal((steps, V))).bfloat16().double().numpy()
    winners = [40 + 7 * j for j in range(steps)]
    for j, w in enumerate(winners):
        rows[j, w] = float(torch.tensor(rows[j].max() + 4.0).bfloat16())
    suppress = [3, 4, 5]
    tokens = np.full((1, 16), 7, dtype=np.int64)
    tokens[0, :P] = [901, 902, 907]
    lp64 = 0.0
    from tests.assist_restatement import processed_row
    for j in range(steps):
        s, _ = processed_row(rows[j], tokens[0, :P + j], P, eos, 0, suppress, ())
        assert int(np.argmax(s)) == winners[j]
        m = s.max()
        lp64 += s[winners[j]] - (m + np.log(np.exp(s - m).sum()))
        tokens[0, P + j] = winners[j]
    from distil_whisper_amd.decoding import token_mask
    kw = dict(suppress=token_mask(suppress, V, DEV, torch.uint8), eos=eos)
    lg = padded_logits(rows, V, ld)
    toks = torch.full((1, 16), 7, dtype=torch.long, device=DEV)
    toks[0, :P] = torch.tensor([901, 902, 907], device=DEV)
    st = torch.tensor([[P], [P], [P + steps + 1], [0]], dtype=torch.int32, device=DEV)
    done, cur = torch.zeros(1, dtype=torch.bool, device=DEV), torch.zeros((1, 1), dtype=torch.long, device=DEV)
    lp, nsp, pos = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    for j in range(steps):
        ops.slot_step(lg[j:j + 1], V, toks, st[0], st[1], st[2], done, st[3], cur, lp_sum=lp, nsp=nsp, nsp_pos=pos, nsp_col=-1, **kw)
    torch.cuda.synchronize()
    assert toks.cpu().numpy().tolist() == tokens.tolist() and st[0].item() == P + steps and not bool(done[0])
    _, _, logprob = ops.score_tokens(lg, V, toks, P, steps, want_scores=False, **kw)
    s64 = []
    for j in range(steps):
        s, _ = processed_row(rows[j], tokens[0, :P + j], P, eos, 0, suppress, ())
        m = s.max()
        s64.append(s[winners[j]] - (m + np.log(np.exp(s - m).sum())))
    one = max(abs(float(logprob[0, j]) - s64[j]) for j in range(steps))
    dev = abs(float(lp[0]) - lp64)
    print(f"eight steps: deviation of the sum {dev:.3e}, one step of dw_score_tokens {one:.3e}")
    assert dev <= steps * REORDER * one


def test_slot_step_scores_refusals_write_nothing(ops):
    V, S = 1030, 2
    lg = torch.zeros((S, 1032), dtype=torch.bfloat16, device=DEV)
    tokens = torch.full((S, 8), 3, dtype=torch.long, device=DEV)
    st = torch.full((5, 4), 2, dtype=torch.int32, device=DEV)
    sc_ = torch.full((2, 4), 0.5, dtype=torch.float32, device=DEV)
    done = torch.zeros(S, dtype=torch.bool, device=DEV)
    cur = torch.full((S, 1), 3, dtype=torch.long, device=DEV)
    good = dict(logits=lg.data_ptr(), S=S, V=V, ld=1032, ts_begin=-1, eos=900, tokens=tokens.data_ptr(), tok_ld=8, len=st[0].data_ptr(),
                plen=st[1].data_ptr(), budget=st[2].data_ptr(), done=done.data_ptr(), row_t=st[3].data_ptr(), cur=cur.data_ptr(),
                lp_sum=sc_[0].data_ptr(), nsp=sc_[1].data_ptr(), nsp_pos=st[4].data_ptr(), nsp_col=5)

    def call(**over):
        a = dict(good, **over)
        return ops.lib.dw_slot_step_scores(a["logits"], a["S"], a["V"], a["ld"], None, None, a["ts_begin"], -1, a["eos"], 0, a["tokens"],
                                           a["tok_ld"], a["len"], a["plen"], a["budget"], a["done"], a["row_t"], a["cur"], a["lp_sum"],
                                           a["nsp"], a["nsp_pos"], a["nsp_col"], ops._stream())
    for over in (dict(logits=None), dict(S=0), dict(V=0), dict(ld=1028), dict(ld=1033), dict(logits=lg.data_ptr() + 2), dict(tokens=None),
                 dict(len=None), dict(plen=None), dict(budget=None), dict(done=None), dict(row_t=None), dict(cur=None), dict(tok_ld=1),
                 dict(len=st[0].data_ptr() + 2), dict(ts_begin=1000, eos=-1),
                 dict(lp_sum=None), dict(lp_sum=sc_[0].data_ptr() + 2), dict(nsp_col=V), dict(nsp=None), dict(nsp_pos=None),
                 dict(nsp=sc_[1].data_ptr() + 2), dict(nsp_pos=st[4].data_ptr() + 2)):
        assert call(**over) == EINVAL, over
    torch.cuda.synchronize()
    assert bool((tokens == 3).all()) and bool((st == 2).all()) and bool((cur == 3).all()) and not bool(done.any())
    assert bool((sc_ == 0.5).all())
    assert call(nsp_col=-1, nsp=None, nsp_pos=None) == 0                  # without the column the two arrays are not asked for
    torch.cuda.synchronize()
    assert bool((sc_[1] == 0.5).all())


# ---- the scheduler --------------------------------------------------------------------------------------------------------------
def device_scenario(ops, monkeypatch, width, P=3):
    model, enc = ss.planted_seek_model(ops, P, dtype=torch.bfloat16, width=width)
    feats, max_frames, expected = ss.utterances(2 * model.dims.max_src)
    spy = ss.Spy(monkeypatch, model, enc.to(DEV).bfloat16())
    return model, spy, feats.to(DEV), max_frames, expected


def compare_utterances(got, want, margins):
    tried = exact = 0
    for b, m in enumerate(margins):
        tried += 1
        if m <= EXACT_ULPS:
            print(f"utterance {b}: margin {m:.1f} ulps, not held to equality")
            continue
        ss.same_segments([got[b]], [want[b]])
        exact += 1
    print(f"utterances tried {tried}, compared {exact}, smallest margin {min(margins):.1f} ulps")
    assert exact >= 1 and 2 * (tried - exact) <= tried


@pytest.mark.parametrize("width,key,N,check_every", [(128, 4, 3, 2), (128, 0, 2, 8), (384, 0, 3, 2), (384, 4, 3, 8), (384, 0, 8, 4)])
def test_slot_schedule_equals_the_lockstep_loop_and_graphs_equal_eager(ops, monkeypatch, key7, width, key, N, check_every):
    model, spy, feats, max_frames, expected = device_scenario(ops, monkeypatch, width)
    B = feats.shape[0]
    args, kw = seek_args(feats, max_frames, [ss.INIT] * B), dict(suppress_tokens=gd.SUPPRESS)
    key7(key)
    ss.ulps_spy(monkeypatch, ops, spy.log)
    want = model.seek_decode(*args, **kw)
    assert [len(w) for w in spy.windows_of(B)] == expected
    margins = ss.utterance_margins(spy.log, B)
    runs = {}
    for name, graphs in (("eager", False), ("graphs", True)):
        spy.clear()
        runs[name] = model.seek_decode(*args, slots=N, check_every=check_every, use_graphs=graphs, **kw)
        spy.check_schedule(B, N)
        steps = model.last_seek_stats["steps"]
        dec = [d for k, d in model._seek_slot_decoders.items() if k[-2] is graphs]
        assert len(dec) == 1 and (len(dec[0].graphs) >= 1) == graphs
        if graphs:                                                   # replay over the same buffers
            spy.clear()
            ss.same_segments(model.seek_decode(*args, slots=N, check_every=check_every, use_graphs=True, **kw), runs[name])
            assert dec[0].steps == 2 * steps
    ss.same_segments(runs["eager"], runs["graphs"])
    compare_utterances(runs["graphs"], want, margins)


def test_fp8_cross_kv_on_slots_equals_the_bf16_slots(ops, monkeypatch):
    model, spy, feats, max_frames, expected = device_scenario(ops, monkeypatch, 384)
    B = feats.shape[0]
    args, kw = seek_args(feats, max_frames, [ss.INIT] * B), dict(suppress_tokens=gd.SUPPRESS, slots=3, check_every=2)
    want = model.seek_decode(*args, **kw)
    spy.clear()
    got = model.seek_decode(*args, cross_kv_dtype="fp8", **kw)
    ss.same_segments(got, want)
    spy.check_schedule(B, 3)
    dec = [d for k, d in model._seek_slot_decoders.items() if k[-3] == "fp8"]
    assert len(dec) == 1 and "cross8" in dec[0].cache and sum(len(s) for s in got) >= sum(expected)


def test_thresholds_on_the_device(ops, monkeypatch):
    from oracle.ref_ops import RefOps
    # (width 128: its three kinds of window stand 0.18 apart in average log-probability; at 384 the planted scores are so peaked
    # that all windows lie within 0.001)
    model, spy, feats, max_frames, _ = device_scenario(ops, monkeypatch, 128)
    B = feats.shape[0]
    args, kw = seek_args(feats, max_frames, [ss.INIT] * B), dict(suppress_tokens=gd.SUPPRESS)
    scores, (lp_thr, lp_gap), (ns_thr, ns_gap) = thresholds_from_lockstep(model, args, kw)
    # the lockstep numbers' own bf16 deviation: this device in bf16 against the CPU statement in fp32, same weights
    cpu, enc_cpu = ss.planted_seek_model(RefOps("cpu", lowp=torch.float32), 3, width=128)
    ss.Spy(monkeypatch, cpu, enc_cpu)
    cpu.seek_decode(*seek_args(feats.cpu(), max_frames, [ss.INIT] * B), logprob_threshold=-1e9, no_speech_threshold=2.0, **kw)
    assert [s[:2] for s in cpu.last_window_scores] == [s[:2] for s in scores]
    dev_lp = max(abs(a[2] - b[2]) for a, b in zip(cpu.last_window_scores, scores))
    dev_ns = max(abs(a[3] - b[3]) for a, b in zip(cpu.last_window_scores, scores))
    print(f"logprob gap {lp_gap:.4f} (bf16 deviation {dev_lp:.2e}), no-speech gap {ns_gap:.3e} (bf16 deviation {dev_ns:.2e})")
    assert lp_gap > 4 * dev_lp and ns_gap > 4 * dev_ns
    th = dict(logprob_threshold=lp_thr, no_speech_threshold=ns_thr)
    spy.clear()
    want = model.seek_decode(*args, **th, **kw)
    lock = sorted(model.last_window_scores)
    assert ("decode",) in spy.log
    skipped = [s for s in lock if s[2] < lp_thr and s[3] > ns_thr]
    assert skipped and len(skipped) < len(lock)
    for graphs in (False, True):
        spy.clear()
        got = model.seek_decode(*args, slots=3, check_every=2, use_graphs=graphs, **th, **kw)
        assert ("decode",) not in spy.log
        ss.same_segments(got, want)
        mine = sorted(model.last_window_scores)
        assert [s[:2] for s in mine] == [s[:2] for s in lock]
        assert [(s[2] < lp_thr, s[3] > ns_thr) for s in mine] == [(s[2] < lp_thr, s[3] > ns_thr) for s in lock]
        # both loops state the same two numbers from bf16 logits of their own passes (token steps here, one teacher-forced pass
        # there): each stands within the bf16 deviation measured above of the fp32 value, so the two differ by at most twice it
        d_lp = max(abs(a[2] - b[2]) for a, b in zip(mine, lock))
        d_ns = max(abs(a[3] - b[3]) for a, b in zip(mine, lock))
        print(f"graphs {graphs}: slots against lockstep, average log-probability {d_lp:.2e} (allowed {2 * dev_lp:.2e}), "
              f"no-speech probability {d_ns:.2e} (allowed {2 * dev_ns:.2e})")
        assert d_lp <= 2 * dev_lp and d_ns <= 2 * dev_ns
