"""The beam-search step on the MI355X (`dw_beam_candidates`, `dw_beam_update`; csrc/beam.hip): the kernels against the float64
restatement (tests/beam_restatement.py) on planted logits, and `beam_search_decode` through the kernels against its torch step
(`DW_BEAM_TORCH=1`) on the tiny model and at distil-large-v3 decoder dimensions.

Where the bounds come from.  Planted logits (tests/beam_cases.py) keep every accumulated score that a selection compares at least
0.25 apart, so integers are decided by the restatement before the kernel runs and must be equal.  Scores: the kernel's deviation
from float64 may be four times the deviation of the torch fp32 step on the same inputs (the largest over the case), never less
than one fp32 ulp of the value itself.  Kernel path against torch path on a model: tokens equal, hypothesis scores within twice the bf16 deviation
that tests/golden/beam_thresholds.json records for the reference's `sequences_scores` (the smallest of its groups); each
comparison prints the figure it found.  The fixture's scenarios run through HipOps as they run on the CPU."""
import numpy as np
import pytest
import torch

import beam_cases as bc
import beam_restatement as br
import history_restatement as hr
from oracle import gen_golden_decode as gd
from test_beam_step import close_scores, to_torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from distil_whisper_amd.ops_hip import HipOps
    return HipOps("cuda:0")


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def run_kernels(ops, st, logits, ld, *, k, V, cur, P, max_length, eos, early_stopping, length_penalty, min_new_tokens=0,
                suppress=None, begin_suppress=None, ts_begin=-1, max_initial=-1, stop0=0):
    """One candidates + update call on the device -> (state as numpy, src_rows, next_tok, stop, cand_val, cand_tok)."""
    dev = "cuda"
    B = st["running"].shape[0]
    R, K = B * k, 2 * k
    t = to_torch(st, dev, lengths_dtype=torch.int32)
    t["unsat"] = t["unsat"][:, 0].contiguous()
    lg = torch.zeros((R, ld), dtype=torch.bfloat16, device=dev)
    lg[:, :V] = torch.from_numpy(logits).to(torch.bfloat16).to(dev)
    fill = eos
    out = dict(running=torch.full_like(t["running"], fill), sequences=torch.full_like(t["sequences"], fill))
    cand_val = torch.full((R, K), float("nan"), dtype=torch.float32, device=dev)
    cand_tok = torch.full((R, K), -7, dtype=torch.int32, device=dev)
    stop = torch.tensor([stop0], dtype=torch.int32, device=dev)
    src_rows = torch.full((R,), -1, dtype=torch.long, device=dev)
    next_tok = torch.full((R,), -1, dtype=torch.long, device=dev)
    plan = torch.empty((4 * R,), dtype=torch.int32, device=dev)
    m = lambda a: None if a is None else torch.from_numpy(a.astype(np.uint8)).to(dev)
    ops.beam_candidates(lg, V, t["running"].view(R, -1), cur, t["run_scores"], cand_val, cand_tok, stop, suppress=m(suppress),
                        begin_suppress=m(begin_suppress), first=(cur == P), no_eos=(cur - P) < min_new_tokens, ts_begin=ts_begin,
                        max_initial=max_initial, begin_index=P, eos=eos)
    hyp_len = (max_length - P) if (early_stopping == "never" and length_penalty > 0.0) else (cur + 1 - P)
    ops.beam_update(cand_val, cand_tok, B, k, V, cur, P, max_length, eos, early_stopping, float((cur + 1 - P) ** length_penalty),
                    float(hyp_len ** length_penalty), t["running"], out["running"], t["sequences"], out["sequences"],
                    t["run_scores"], t["beam_scores"], t["finished"], t["lengths"], t["unsat"], stop, src_rows, next_tok, plan)
    torch.cuda.synchronize()
    got = {n: (out[n] if n in out else t[n]).cpu().numpy() for n in t}
    return got, src_rows.cpu().numpy(), next_tok.cpu().numpy(), bool(stop.item()), cand_val.cpu().numpy(), cand_tok.cpu().numpy()


def check_case(ops, rng, *, B, k, V, ld, kind="text", ts=False, first=False, n_fin=0, early=False, lp=1.0, last=False, min_new=0,
               regions=None, top_cols=None, max_initial=-1, masks=False, unsat_off=False, expect_stop=None, fin_scores=None):
    lay = bc.layout(V)
    P = 3
    cur = P if first else P + 6
    L = cur + 1 if last else cur + 5
    st = bc.make_state(rng, B, k, L, P, cur, lay, kind=kind, n_finished=n_fin, first=first)
    if unsat_off:
        st["unsat"][0] = False
    if fin_scores is not None:
        st["beam_scores"][:, :n_fin] = fin_scores
    regions = regions or [(0, lay["eos"])]
    logits, run = bc.planted_logits(rng, st, k, V, lay, regions, top_cols, keep_run=first)
    st["run_scores"] = run
    sup = bsup = None
    if masks:                                            # a third of the text ids, and so of the planted text columns, is masked
        sup = np.zeros(V, dtype=bool); sup[:lay["eos"] // 3] = True; sup[lay["tb"] + 20:lay["tb"] + 30] = True
        bsup = np.zeros(V, dtype=bool); bsup[[lay["eos"], lay["eos"] // 3 + 5]] = True
    kw = dict(k=k, V=V, cur=cur, P=P, max_length=L, eos=lay["eos"], early_stopping=early, length_penalty=lp, min_new_tokens=min_new,
              suppress=sup, begin_suppress=bsup, ts_begin=lay["tb"] if ts else -1, max_initial=max_initial)
    want, src_rows, next_tok, stop, cand = br.step_ref(st, logits, **kw)
    # the case really is decided: K + 1 finite candidates per utterance, everything compared at least 0.2 apart
    live = (st["run_scores"] > -1.0e8).reshape(-1)
    merged = np.sort(np.where(live[:, None], cand[0], -np.inf).reshape(B, -1), axis=1)[:, ::-1][:, :2 * k + 1]
    assert np.all(np.isfinite(merged[:, :2 * k])) and np.min(-np.diff(merged[:, :2 * k], axis=1)) > 0.2
    assert np.min(cand[2]) > 0.2
    if expect_stop is not None:
        assert stop == expect_stop
    got, g_src, g_next, g_stop, cv, ct = run_kernels(ops, st, logits, ld, **kw)
    # ---- integers: exact ----
    assert np.array_equal(ct[live], cand[1][live])
    assert g_stop == stop
    assert np.array_equal(g_src, src_rows) and np.array_equal(g_next, next_tok)
    for name in ("running", "sequences", "finished", "lengths", "unsat"):
        assert np.array_equal(got[name], want[name]), name
    # ---- scores: against the torch fp32 step on the same inputs ----
    from distil_whisper_amd import decoding
    tr = dict(begin_index=P, no_timestamps_token_id=lay["nots"],
              max_initial_timestamp_index=None if max_initial < 0 else max_initial) if ts else None
    cfg = dict(P=P, max_length=L, nb=k, V=V, eos=lay["eos"], min_new_tokens=min_new, length_penalty=lp, early_stopping=early,
               sup=None if sup is None else torch.from_numpy(sup).cuda(), bsup=None if bsup is None else torch.from_numpy(bsup).cuda(),
               timestamp_rules=tr)
    tst = to_torch(st, "cuda")
    t_src, go_on = decoding.beam_step_torch(tst, torch.from_numpy(logits).to(torch.bfloat16).cuda(), cur, cfg)
    assert bool(go_on) == (not stop) and np.array_equal(t_src.cpu().numpy(), src_rows)
    assert np.array_equal(tst["running"].cpu().numpy(), want["running"])
    worst = 0.0
    for name in ("run_scores", "beam_scores"):
        ref = want[name]
        real = ref > -1.0e8
        torch_dev = np.abs(tst[name].cpu().numpy().astype(np.float64) - ref)[real]
        kern_dev = np.abs(got[name].astype(np.float64) - ref)[real]
        if real.any():
            bound = np.maximum(4.0 * torch_dev.max(), ulp32(ref[real]))
            print(f"{name}: kernel {kern_dev.max():.3e} torch {torch_dev.max():.3e} ulp {ulp32(ref[real]).max():.3e}")
            assert np.all(kern_dev <= bound), (name, kern_dev.max(), torch_dev.max())
            worst = max(worst, kern_dev.max())
        close_scores(got[name], ref, 1.0)                # (the -1e9 sentinels)
    fin = np.isfinite(cand[0]) & live[:, None]
    assert np.all(np.abs(cv.astype(np.float64) - cand[0])[fin] <= 4 * ulp32(np.abs(cand[0][fin]) + 128.0))
    assert np.all(np.isneginf(cv[live][~np.isfinite(cand[0][live])]))
    return st, want, stop


SHAPES = [(1030, 1032), (51865, 51872), (51866, 51868)]


@pytest.mark.parametrize("V,ld", SHAPES)
@pytest.mark.parametrize("k", [2, 3, 5, 8])
@pytest.mark.parametrize("B", [1, 3])
def test_kernels_against_the_restatement_on_every_shape(ops, V, ld, k, B):
    rng = np.random.default_rng(V + 100 * k + B)
    lay = bc.layout(V)
    check_case(ops, rng, B=B, k=k, V=V, ld=ld, n_fin=1, masks=True)
    check_case(ops, rng, B=B, k=k, V=V, ld=ld, kind="open", ts=True, regions=[(lay["tb"] + 8, V), (0, lay["eos"])], masks=True)


@pytest.mark.parametrize("k", [3, 8])
def test_kernels_against_the_restatement_beyond_53248_columns(ops, k):
    """The 16-chunk form of the candidates kernel (vocabularies of 53 249 .. 65 536 columns)."""
    V, ld = 53252, 53312
    rng = np.random.default_rng(V + k)
    lay = bc.layout(V)
    check_case(ops, rng, B=1, k=k, V=V, ld=ld, n_fin=1, masks=True)
    check_case(ops, rng, B=1, k=k, V=V, ld=ld, kind="open", ts=True, regions=[(lay["tb"] + 8, V), (0, lay["eos"])], masks=True)


STATES = {
    "first step": dict(first=True, masks=True),
    "timestamps: first token": dict(first=True, ts=True, regions="ts"),
    "timestamps: first token, max_initial": dict(first=True, ts=True, regions="ts_initial", max_initial=120),
    "timestamps: text + timestamp": dict(kind="text_ts", ts=True, regions="both"),
    "timestamps: closed pair": dict(kind="pair", ts=True, regions="both"),
    "timestamps: mass rule taken": dict(kind="open", ts=True, regions="both_ts_first"),
    "timestamps: mass rule not taken": dict(kind="open", ts=True, regions="text"),
    "no_eos": dict(min_new=100, eos_rank=0),
    "EOS among the first k": dict(eos_rank=0, n_fin=1),
    "EOS among the second k": dict(eos_rank=1, n_fin=1),
    "last step": dict(last=True, n_fin=1, expect_stop=True),
    "length_penalty 0.5": dict(lp=0.5, eos_rank=0, n_fin=2),
    "length_penalty 2.0": dict(lp=2.0, eos_rank=0, n_fin=2),
    "early_stopping False flips stop": dict(early=False, n_fin="all", fin_scores=-0.001, expect_stop=True),
    "early_stopping False goes on": dict(early=False, n_fin="all", fin_scores=-1.0e6, expect_stop=False),
    "early_stopping True flips stop": dict(early=True, n_fin="all_but_one", eos_rank=0, fin_scores=-1.0e6, expect_stop=True),
    "early_stopping True goes on": dict(early=True, n_fin=0, eos_rank=1, expect_stop=False),
    "early_stopping never flips stop": dict(early="never", lp=2.0, n_fin="all", fin_scores=-0.001, expect_stop=True),
    "early_stopping never goes on": dict(early="never", lp=2.0, n_fin="all", fin_scores=-1.0e6, expect_stop=False),
    "an utterance already satisfied": dict(unsat_off=True, eos_rank=0, n_fin=1),
}


@pytest.mark.parametrize("name", list(STATES))
@pytest.mark.parametrize("V,ld,k,B", [(1030, 1032, 3, 3), (51866, 51868, 5, 1)])
def test_kernels_against_the_restatement_in_every_state(ops, name, V, ld, k, B):
    rng = np.random.default_rng(sorted(STATES).index(name) * 7 + V + k)
    lay = bc.layout(V)
    a = dict(STATES[name])
    reg = a.pop("regions", "text")
    a["regions"] = {"text": [(0, lay["eos"])], "ts": [(lay["tb"], V)], "ts_initial": [(lay["tb"], lay["tb"] + 121)],
                    "both": [(0, lay["eos"]), (lay["tb"] + 8, V)], "both_ts_first": [(lay["tb"] + 8, V), (0, lay["eos"])]}[reg]
    rank = a.pop("eos_rank", None)
    if rank is not None:         # beam 0's planted value of that rank sits in its EOS column: merged position k - 1 (rank 0) / 2k - 1
        a["top_cols"] = {u * k: {rank: lay["eos"]} for u in range(B)}
    a["n_fin"] = {"all": k, "all_but_one": k - 1}.get(a.get("n_fin", 0), a.get("n_fin", 0))
    st, want, stop = check_case(ops, rng, B=B, k=k, V=V, ld=ld, **a)
    eos = lay["eos"]
    new_fin = want["finished"].sum() - st["finished"].sum()
    if name in ("EOS among the first k", "length_penalty 0.5", "length_penalty 2.0", "early_stopping True flips stop"):
        assert new_fin > 0 or want["lengths"].max() == 7          # a hypothesis finished at this step
    if name in ("no_eos", "EOS among the second k", "early_stopping True goes on"):
        assert new_fin == 0 and not (want["running"][:, :, 9] == eos).any()


def test_a_call_with_stop_set_leaves_the_state_as_it_is(ops):
    rng = np.random.default_rng(5)
    B, k, V, ld, P, cur, L = 3, 3, 1030, 1032, 3, 9, 14
    lay = bc.layout(V)
    st = bc.make_state(rng, B, k, L, P, cur, lay, n_finished=2)
    logits, run = bc.planted_logits(rng, st, k, V, lay, [(0, lay["eos"])])
    st["run_scores"] = run
    got, src, nxt, stop, cv, ct = run_kernels(ops, st, logits, ld, k=k, V=V, cur=cur, P=P, max_length=L, eos=lay["eos"],
                                              early_stopping=False, length_penalty=1.0, stop0=1)
    assert stop and np.array_equal(src, np.arange(B * k)) and np.all(nxt == -1)
    assert np.all(np.isnan(cv)) and np.all(ct == -7)                 # the candidates entry wrote nothing
    for name in ("running", "sequences", "finished", "lengths", "unsat"):
        assert np.array_equal(got[name], st[name]), name
    for name in ("run_scores", "beam_scores"):
        assert np.array_equal(got[name], st[name].astype(np.float32)), name


# ---- beam_search_decode: kernel path against the torch step --------------------------------------------------------------------
# (8 steps x 4 fp32 roundings x 1.9e-6, the ulp of scores below 32, is 6e-5: no selection can turn on it above this margin)
MIN_MARGIN = 1e-4


def _decode(eng, enc, prompt, monkeypatch, torch_path, margins=None, **kw):
    from distil_whisper_amd import decoding
    monkeypatch.setenv(decoding.BEAM_TORCH_ENV, "1" if torch_path else "0")
    calls = []
    if margins is not None:                              # the accumulated scores the torch step selects from, per step
        real = decoding.beam_step_torch

        def spy(st, logits, cur, cfg):
            margins.append(bc.step_margin(decoding, st, logits, cur, cfg))
            return real(st, logits, cur, cfg)
        monkeypatch.setattr(decoding, "beam_step_torch", spy)
    if not torch_path:
        for name in ("beam_candidates", "beam_update"):
            fn = getattr(type(eng.ops), name)
            monkeypatch.setattr(type(eng.ops), name, lambda self, *a, _f=fn, **k: (calls.append(1), _f(self, *a, **k))[1])
    out = decoding.beam_search_decode(eng, enc, prompt, return_scores=True, **kw)
    monkeypatch.undo()
    return out, calls


def _compare(eng, enc, prompt, monkeypatch, **kw):
    from test_beam_step import GOLD
    (w_seq, w_sc, w_pre), _ = _decode(eng, enc, prompt, monkeypatch, True, **kw)
    (g_seq, g_sc, g_pre), calls = _decode(eng, enc, prompt, monkeypatch, False, **kw)
    assert calls, "the kernel path was not taken"
    assert g_seq.tolist() == w_seq.tolist()
    bound = 2 * min(g["bf16_dev_score"] for g in GOLD["groups"])
    dev = float((g_sc - w_sc).abs().max())
    print(f"scores: kernel path - torch path {dev:.3e}, bound {bound:.3e}")
    assert dev <= bound
    assert torch.equal(g_pre, w_pre)


def _selected(tried, checked):
    """Margin selection must not reject more than half of what it tries: the margin would then be wrong for the model."""
    print(f"inputs tried {tried}, compared {checked}, rejected {tried - checked}")
    assert checked >= 1 and 2 * (tried - checked) <= tried


@pytest.mark.parametrize("k,early,lp,ts", [(2, False, 1.0, False), (3, True, 2.0, True), (5, "never", 0.5, False)])
def test_tiny_model_kernel_path_equals_the_torch_path(ops, monkeypatch, k, early, lp, ts):
    sc = dict(seed=11, ts_fields=ts, B=2, kind="short")
    model = hr.dropin(ops, sc)
    eng = model.engine
    ids = [gd.SOT, gd.LANG["<|en|>"], gd.TRANSCRIBE] + ([] if ts else [gd.NOTIMESTAMPS])
    prompt = torch.tensor([ids] * 2, device="cuda")
    rules = dict(begin_index=len(ids), no_timestamps_token_id=gd.NOTIMESTAMPS, max_initial_timestamp_index=50) if ts else None
    kw = dict(max_new_tokens=8, num_beams=k, eos_token_id=gd.EOS, pad_token_id=gd.EOS, suppress_tokens=gd.SUPPRESS,
              begin_suppress_tokens=gd.BEGIN_SUPPRESS, length_penalty=lp, early_stopping=early, timestamp_rules=rules)
    checked = tried = 0
    for fseed in range(100, 160):                        # margin-selected inputs, as the fixtures of this package are
        enc, _ = eng.encode(gd.features(fseed, 2).cuda().to(torch.float32).contiguous(), save=False)
        margins = []
        tried += 1
        _decode(eng, enc, prompt, monkeypatch, True, margins=margins, **kw)
        if min(margins) < MIN_MARGIN:
            continue
        _compare(eng, enc, prompt, monkeypatch, **kw)
        checked += 1
        if checked == 2:
            break
    _selected(tried, checked)


def test_distil_large_v3_dimensions_kernel_path_equals_the_torch_path(ops, monkeypatch):
    from distil_whisper_amd import student_init as si
    from distil_whisper_amd.engine import WhisperDims
    from distil_whisper_amd.modeling import WhisperForConditionalGeneration
    dims = WhisperDims(1280, 20, 5120, 1, 2, 51866, 128, decoder_start_token_id=50258)
    B, k, new = 2, 5, 8
    prompt = torch.tensor([[50258, 50259, 50360, 50364]] * B, device="cuda")
    kw = dict(max_new_tokens=new, num_beams=k, eos_token_id=50257, pad_token_id=50257, min_new_tokens=2,
              suppress_tokens=list(range(1, 90)) + list(range(50258, 50364)), begin_suppress_tokens=[220, 50257])
    model = WhisperForConditionalGeneration(dims, ops=ops, state_dict=si.random_state_dict(dims, 0, "cuda", std=0.05))
    eng = model.engine
    checked = tried = 0
    for seed in range(60):                               # margin-selected encoder states, as the fixtures of this package are
        g = torch.Generator().manual_seed(seed)
        enc = (torch.randn(B, dims.max_src, dims.d_model, generator=g) * 0.5).cuda().reshape(-1, dims.d_model).to(eng.lowp).contiguous()
        margins = []
        tried += 1
        _decode(eng, enc, prompt, monkeypatch, True, margins=margins, **kw)
        if min(margins) < MIN_MARGIN:
            continue
        _compare(eng, enc, prompt, monkeypatch, **kw)
        checked += 1
        if checked == 2:
            break
    _selected(tried, checked)


def _gold_groups():
    from test_beam_step import GOLD
    return GOLD["groups"]


@pytest.mark.parametrize("gi", range(len(_gold_groups())))
def test_fixture_scenarios_through_the_kernels(ops, monkeypatch, gi):
    """tests/golden/beam_thresholds.json through HipOps: the reference's tokens and segments in every scenario (thresholds between
    the windows' observed scores / no-speech probabilities, four bf16 deviations away from each)."""
    import test_beam_step as tbs
    from distil_whisper_amd import decoding
    monkeypatch.setenv(decoding.BEAM_TORCH_ENV, "0")
    g = _gold_groups()[gi]
    model = tbs.fixture_model(g, ops)
    calls = []
    real = type(ops).beam_update
    monkeypatch.setattr(type(ops), "beam_update", lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    for s in g["scenarios"]:
        feats, kw = tbs.fixture_call(g, s["thresholds"], "cuda")
        mine = model.generate(feats, return_segments=True, **kw)
        tbs.same_as_fixture(dict(sequences=mine["sequences"].cpu(), segments=mine["segments"]), s["sequences"], s["segments"])
    assert calls
