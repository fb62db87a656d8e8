"""TEST INFRASTRUCTURE -- the timestamp seek loop on slots (tests/test_seek_slots*.py): a planted model whose windows end where the
test says, utterances whose every frame names its window, spies on the encoder and the schedule, and the float64 restatement of the
two numbers `dw_slot_step_scores` keeps.

The model is tests/assist_rows_cases.planted_pair's target (the recipe of tests/test_slots.planted_target) with a generated
sequence under the timestamp rules:

    SEQ = <0.00> x1 x2 <0.80> <0.80> x3 <1.20> EOS          (index 5 is planted weak)

A window of kind 0 / 1 emits all of it: it ends with a single timestamp, so the utterance moves past the window.  A window of kind 2
takes EOS at the weak index: it ends with the closed pair <0.80> <0.80>, so the utterance moves 80 frames.  The encoder is replaced
by one that reads the window's kind, utterance and first frame from mel channels 0 / 1 / 2 of the window's first frame and returns
the planted encoder rows of that kind: which window follows which is then decided by the decoded tokens alone."""
import numpy as np
import torch

from oracle import gen_golden_decode as gd
from tests import assist_rows_cases as arc
from tests.assist_restatement import processed_row

TB = gd.NOTIMESTAMPS + 1
T_PAIR, T_LAST = TB + 40, TB + 60
PAIR_FRAMES = 80                                                        # what a closed pair <0.80> <0.80> moves an utterance by
SEQ = [TB, 50, 61, T_PAIR, T_PAIR, 72, T_LAST, gd.EOS]
WEAK = (5,)
ROW_TOKENS = [400, 410, gd.EOS]
MAX_NEW = 10
RULES = dict(no_timestamps_token_id=gd.NOTIMESTAMPS, max_initial_timestamp_index=50)
INIT = [gd.SOT, gd.LANG["<|en|>"], gd.TRANSCRIBE]
MIN_KEEP = 0.24                                                         # every decision keeps this share of the best score
SEEDS = {128: 22, 384: 21}                                              # (chosen on the CPU statement in fp32: both keep it)


def planted_seek_model(ops, P, seed=None, dtype=torch.float32, width=128):
    """-> (model planted for decoder prompts of P tokens, enc rows of the three kinds [3 * max_src, d_model])."""
    from distil_whisper_amd import student_init as si
    from distil_whisper_amd.engine import WhisperDims
    from distil_whisper_amd.modeling import WhisperForConditionalGeneration
    seed = SEEDS[width] if seed is None else seed
    cfg = WhisperDims(width, width // 64, 4 * width, 1, 2, gd.V, 80, max_src=128, pad_token_id=gd.EOS, decoder_start_token_id=gd.SOT)
    sd = {k: v.cpu() for k, v in si.random_state_dict(cfg, seed, "cpu").items()}
    sd, _, enc = arc.planted_pair(sd, P, SEQ, WEAK, ROW_TOKENS, cfg.d_model, cfg.max_src, scale=4.0, head_gain=4.0)
    return WhisperForConditionalGeneration(cfg, ops=ops, state_dict=sd, dtype=dtype), enc


def utterances(W, n=None):
    """-> (features f32 [B, 80, frames], max_frames, windows expected per utterance).  Per utterance a list of (first frame, kind):
    the kind of every window that starts at or behind that frame."""
    plan = [(250, [(0, 0)], 1),                                         # one window: a single timestamp ends it
            (230, [(0, 2)], 3),                                         # closed pairs: 0 -> 80 -> 160 -> 240
            (W, [(0, 2), (80, 1)], 2),                                  # a closed pair, then the rest in one window
            (W + 144, [(0, 0), (W, 2), (W + 80, 1)], 3),                # longer than a window
            (100, [(0, 1)], 1),
            (170, [(0, 2), (160, 0)], 3),
            (90, [(0, 2), (80, 0)], 2)]
    plan = plan[:n] if n is not None else plan
    frames = max(p[0] for p in plan)
    feats = torch.zeros(len(plan), 80, frames)
    for b, (mf, kinds, _) in enumerate(plan):
        for t0, k in kinds:
            feats[b, 0, t0:] = float(k)
        feats[b, 1] = float(b)
        feats[b, 2] = torch.arange(frames, dtype=torch.float32)
        feats[b, :, mf:] = 0.0
    return feats, [p[0] for p in plan], [p[2] for p in plan]


class Spy:
    """Replaces `engine.encode` by the planted encoder and logs, in order: ("enc", [(utterance, first frame), ...]) per encoder
    call, ("seg", tokens) per `retrieve_segment`, ("end", utterance) per window a SlotDecoder hands back, ("decode",) per
    teacher-forced `engine.decode` pass."""

    def __init__(self, monkeypatch, model, enc):
        from distil_whisper_amd import generation as G
        from distil_whisper_amd.decoding import SlotDecoder
        self.log = []
        eng, S = model.engine, model.dims.max_src
        kinds = enc.view(3, S, -1)

        def encode(feats, save=False, **kw):
            head = feats[:, :3, 0].round().long().tolist()
            self.log.append(("enc", [(u, t) for _, u, t in head]))
            return torch.cat([kinds[k] for k, _, _ in head]).to(eng.lowp).contiguous(), None
        monkeypatch.setattr(eng, "encode", encode, raising=False)
        seg, run, decode = G.retrieve_segment, SlotDecoder.run, eng.decode

        def retrieve(seq, *a, **k):
            self.log.append(("seg", list(seq)))
            return seg(seq, *a, **k)
        monkeypatch.setattr(G, "retrieve_segment", retrieve)

        def spy_run(dec, windows):
            for res in run(dec, windows):
                self.log.append(("end", res[0]))
                yield res
        monkeypatch.setattr(SlotDecoder, "run", spy_run)

        def spy_decode(*a, **k):
            self.log.append(("decode",))
            return decode(*a, **k)
        monkeypatch.setattr(eng, "decode", spy_decode, raising=False)

    def clear(self):
        del self.log[:]

    def encoder_batches(self):
        return [len(e[1]) for e in self.log if e[0] == "enc"]

    def windows_of(self, B):
        out = [[] for _ in range(B)]
        for e in self.log:
            if e[0] == "enc":
                for u, t in e[1]:
                    out[u].append(t)
        return out

    def passes(self):
        """The lockstep loop's passes: per encoder call the token lists its windows gave."""
        out = []
        for e in self.log:
            if e[0] == "enc":
                out.append([])
            elif e[0] == "seg":
                out[-1].append(e[1])
        return out

    def check_schedule(self, B, N):
        """No utterance is encoded for a window before its previous window has ended; never more than 2 N encoded windows held."""
        open_, held, most = [False] * B, 0, 0
        for e in self.log:
            if e[0] == "enc":
                assert len(e[1]) <= N
                for u, _ in e[1]:
                    assert not open_[u], (u, "encoded again before its window ended")
                    open_[u] = True
                held += len(e[1])
                most = max(most, held)
            elif e[0] == "end":
                assert open_[e[1]]
                open_[e[1]] = False
                held -= 1
        assert not any(open_) and held == 0
        assert most <= 2 * N, (most, N)
        return most


def margin_spy(monkeypatch):
    """Records, for every row `decoding.processed_scores` judges from now on, (best - runner-up) / |best|."""
    from distil_whisper_amd import decoding
    seen = []
    orig = decoding.processed_scores

    def spy(*a, **k):
        sc = orig(*a, **k)
        top = sc.float().topk(2, -1).values
        seen.extend(((top[:, 0] - top[:, 1]) / top[:, 0].abs()).tolist())
        return sc
    monkeypatch.setattr(decoding, "processed_scores", spy)
    return seen


def same_segments(got, want):
    assert len(got) == len(want)
    for g_row, w_row in zip(got, want):
        assert [list(s["tokens"]) for s in g_row] == [list(s["tokens"]) for s in w_row]
        for g, w in zip(g_row, w_row):
            assert abs(float(g["start"]) - float(w["start"])) < 1e-9 and abs(float(g["end"]) - float(w["end"])) < 1e-9


# ---- dw_slot_step_scores ----------------------------------------------------------------------------------------------------------
def _lse(x):
    m = np.max(x)
    return m + np.log(np.sum(np.exp(x - m))) if np.isfinite(m) else -np.inf


def scores_launch(c, nsp_col):
    """The launch of slots_cases.make_launch `c` with three more slots, and the two numbers in float64 (include/dwamd.h,
    dw_slot_step_scores): a copy of the forced slot whose nsp_pos is elsewhere, and copies of a first-position slot behind a prompt
    of ONE token (the first generated step reads the no-speech probability off the processed row) and of the EOS slot.
    -> dict(c's arrays extended, nsp_pos, lp0 / nsp0: what the buffers hold before, lp / nsp: after, gen: the generated slots)."""
    from tests import slots_cases as sc
    at = {n: i for i, n in enumerate(c["names"])}
    first = at["ts_first"] if c["ts"] is not None else at["first"]
    rows = list(range(len(c["names"]))) + [at["prompt"], first, at["eos"]]
    names = list(c["names"]) + ["prompt_elsewhere", "first_p1", "eos_copy"]
    ext = {k: np.array(c[k])[rows].copy() for k in ("logits", "tokens", "length", "plen", "budget", "done")}
    S = len(rows)
    b = names.index("first_p1")
    ext["length"][b], ext["plen"][b], ext["budget"][b] = 1, 1, 10       # tokens[b][0] is the whole prompt
    nsp_pos = (ext["plen"] - 1).astype(np.int64)                         # default: the first generated step
    nsp_pos[names.index("prompt")] = 1                                   # the forced step of this launch (length 2: row of input 1)
    nsp_pos[names.index("prompt_elsewhere")] = 3
    kw = dict(eos=c["eos"], min_new=c["min_new"], suppress=c["suppress"], begin_suppress=c["begin_suppress"], ts=c["ts"])
    if nsp_col >= 0:
        # the no-speech column stands one below the best score of the rows it is read from, so that the probability is of order
        # 0.1 and a wrong column, a wrong row or a zero is far outside any rounding (one below: the pick keeps its 0.25)
        for name in ("prompt", "prompt_elsewhere", "first_p1"):
            i = names.index(name)
            n, P = int(ext["length"][i]), int(ext["plen"][i])
            best = ext["logits"][i].max() if n < P else processed_row(ext["logits"][i], ext["tokens"][i, :n], P, c["eos"], c["min_new"],
                                                                       c["suppress"], c["begin_suppress"], c["ts"])[0].max()
            ext["logits"][i, nsp_col] = float(torch.tensor(best - 1.0).bfloat16())
    want = sc.slot_step_ref(ext["logits"], ext["tokens"], ext["length"], ext["plen"], ext["budget"], ext["done"], **kw)
    lp0 = -0.25 * np.arange(1, S + 1, dtype=np.float64)                  # (sums of earlier steps; exact in fp32)
    nsp0 = np.full(S, 0.625)
    lp, nsp, gen = lp0.copy(), nsp0.copy(), []
    for i in range(S):
        n, P = int(ext["length"][i]), int(ext["plen"][i])
        if ext["done"][i]:
            continue
        if n >= P:
            s, _ = processed_row(ext["logits"][i], ext["tokens"][i, :n], P, c["eos"], c["min_new"], c["suppress"], c["begin_suppress"],
                                 c["ts"])
            nxt = int(want[0][i, n])
            assert nxt == int(np.argmax(s))
            lp[i] += s[nxt] - _lse(s)
            gen.append(i)
            if nsp_col >= 0 and n - 1 == nsp_pos[i]:
                nsp[i] = np.exp(s[nsp_col] - _lse(s))
        elif nsp_col >= 0 and n - 1 == nsp_pos[i]:
            nsp[i] = np.exp(ext["logits"][i][nsp_col] - _lse(ext["logits"][i]))
    # what the launch was planted for
    touched = [i for i in range(S) if nsp[i] != nsp0[i]]
    if nsp_col >= 0:
        assert names.index("prompt") in touched and names.index("first_p1") in touched
        assert nsp[names.index("prompt")] > 0.05                        # a probability a wrong value cannot hide behind
        if c["ts"] is None:
            assert nsp[names.index("first_p1")] > 0.05
        else:
            assert nsp[names.index("first_p1")] == 0.0                  # the first token is a timestamp: the column is excluded
        assert not {names.index(x) for x in ("prompt_elsewhere", "done", "eos", "eos_copy")} & set(touched)
    else:
        assert not touched
    assert lp[names.index("done")] == lp0[names.index("done")] and lp[names.index("prompt")] == lp0[names.index("prompt")]
    assert int(want[0][names.index("eos"), ext["length"][names.index("eos")]]) == c["eos"] and names.index("eos") in gen
    if c["ts"] is not None:
        i = names.index("ts_mass_taken")
        assert int(want[0][i, ext["length"][i]]) >= c["ts"]["no_timestamps_token_id"] + 1
    return dict(ext, names=names, nsp_pos=nsp_pos, lp0=lp0, nsp0=nsp0, lp=lp, nsp=nsp, gen=gen, want=want, **kw)


def ulps_spy(monkeypatch, ops, log):
    """Appends ("sel", [margin per row]) to `log` for every generated step of the lockstep loop's `greedy_select`: the gap between
    the selection and the runner-up in bf16 ulps of the best score (inf for a row that has ended) -- the measure of
    tests/test_slots_gpu.margins_of_greedy, for every row of the pass."""
    from distil_whisper_amd.decoding import processed_scores
    orig = type(ops).greedy_select

    def spy(self, logits, V, tokens, n, cur, **k):
        if not k.get("forced"):
            r = None if k.get("ts_begin", -1) < 0 else dict(no_timestamps_token_id=k["ts_begin"] - 1,
                                                            max_initial_timestamp_index=None if k["max_initial"] < 0 else k["max_initial"])
            s = processed_scores(logits[:tokens.shape[0], :V], tokens, n, begin_index=k.get("begin_index", 1), eos=k.get("eos"),
                                 no_eos=k.get("no_eos", False), first=k.get("first", False), suppress=k.get("suppress"),
                                 begin_suppress=k.get("begin_suppress"), timestamp_rules=r)
            top = s.float().topk(2, -1).values
            m = (top[:, 0] - top[:, 1]) / torch.exp2(torch.floor(torch.log2(top[:, 0].abs().clamp(min=1e-30))) - 7)
            m = torch.where(k["done"][:tokens.shape[0]].bool(), torch.full_like(m, float("inf")), m)
            log.append(("sel", m.tolist()))
        return orig(self, logits, V, tokens, n, cur, **k)
    monkeypatch.setattr(type(ops), "greedy_select", spy)


def utterance_margins(log, B):
    """The smallest margin of every utterance over the lockstep run logged by Spy + ulps_spy."""
    worst, rows = [float("inf")] * B, []
    for e in log:
        if e[0] == "enc":
            rows = [u for u, _ in e[1]]
        elif e[0] == "sel":
            for u, m in zip(rows, e[1]):
                worst[u] = min(worst[u], m)
    return worst
