"""Token-level timestamps on the MI355X: each alignment kernel (csrc/align.hip) against its restatement on exactly the input the
kernel saw -- the stage before it copied to the host, so that one stage is compared at a time --, then `generate(
return_token_timestamps=True)` end to end on the scenarios of tests/golden/token_timestamps.json.

Where the bounds come from:
  * probabilities: the project's attention test (tests/test_kernels_gpu.py: relerr < 1e-2 on bf16 operands), rows sum to 1 within 2e-3;
  * normalise / filter / average: measured, not chosen -- the kernel's largest error against a float64 evaluation may be at most
    4 x that of the fp32 torch restatement against the same float64 (another summation order and a division where torch
    multiplies by a reciprocal are worth about a factor of two each);
  * DTW: none.  The path is a function of comparisons between fp32 sums the kernel forms exactly as the reference does;
  * end to end: the timestamps must EQUAL what the reference's DTW function makes of the cost matrix the GPU produced (plumbing, no
    tolerance), and against the fp32 fixture the share of tokens more than one frame (0.02 s) away is at most
    max(2 x ref_bf16_share, one token): as close to the fp32 reference as twice the reference's own bf16 run is
    (the rule of tests/test_sharp_parity_gpu.py).  Every position of `token_timestamps` counts."""
import numpy as np
import pytest
import torch

import align_restatement as ar

pytestmark = pytest.mark.gpu

GOLD = ar.gold()
META = GOLD["meta"]
SC = {s["name"]: s for s in GOLD["scenarios"]}
FRAME = 0.02


@pytest.fixture(scope="module")
def ops():
    from distil_whisper_amd.ops_hip import HipOps
    return HipOps("cuda:0")


def relerr(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _qk(B, L, H, kv_rows, seed, scale=1.0):
    """q / k as column slices of wider buffers with padded row pitches"""
    g = torch.Generator().manual_seed(seed)
    D = H * 64
    qbuf = (torch.randn(B * L, 3 * D + 64, generator=g) * scale).to(torch.bfloat16).cuda()
    kbuf = (torch.randn(B * kv_rows, 2 * D + 64, generator=g) * scale).to(torch.bfloat16).cuda()
    return qbuf[:, D:2 * D], kbuf[:, :D]


def _probs(ops, q, k, heads, B, L, Lk, kv_rows):
    """all the listed heads through two calls that fill neighbouring slots"""
    n = len(heads)
    probs = torch.full((B, n, L, 1504), -7.0, dtype=torch.float32, device="cuda")
    cut = max(1, n // 2)
    hd = torch.tensor(heads, dtype=torch.int32, device="cuda")
    ops.cross_attn_probs(q, k, hd[:cut].contiguous(), probs, 0, B, L, Lk, kv_batch_rows=kv_rows)
    if cut < n:
        ops.cross_attn_probs(q, k, hd[cut:].contiguous(), probs, cut, B, L, Lk, kv_batch_rows=kv_rows)
    torch.cuda.synchronize()
    return probs


# ---- 5 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L,n", [(1, 1, 1), (2, 27, 3), (3, 223, 6), (16, 447, 6)])
def test_cross_attn_probs(ops, B, L, n):
    H, Lk, kv_rows = 8, 1500, 1536
    q, k = _qk(B, L, H, kv_rows, seed=50 + L)
    heads = [7, 0, 3, 5, 2, 6][:n]
    probs = _probs(ops, q, k, heads, B, L, Lk, kv_rows)
    ref = ar.probs_ref(q.cpu(), k.cpu(), heads, B, L, Lk, kv_rows)
    got = probs[..., :Lk].cpu()
    print(f"probs B={B} L={L} n={n}: relerr {relerr(got, ref):.3e}  max |rowsum - 1| {(got.sum(-1) - 1).abs().max().item():.3e}")
    assert relerr(got, ref) < 1e-2
    assert (got.sum(-1) - 1).abs().max().item() < 2e-3
    assert (probs[..., Lk:] == -7.0).all()                    # nothing written behind the valid keys


def test_cross_attn_probs_spiked_row(ops):
    B, L, H, Lk = 1, 5, 2, 1500
    q = torch.zeros(B * L, H * 64)
    k = torch.randn(Lk, H * 64, generator=torch.Generator().manual_seed(4)) * 0.1
    q[2, 64:128] = 1.0
    k[:, 64:128] = 0.0
    k[777, 64:128] = 30.0 * 8 / 64                            # score 0.125 * 64 * 3.75 = 30 above the other keys' 0
    q, k = q.to(torch.bfloat16).cuda(), k.to(torch.bfloat16).cuda()
    probs = _probs(ops, q, k, [1], B, L, Lk, Lk)[..., :Lk].cpu()
    assert torch.isfinite(probs).all()
    assert probs[0, 0, 2, 777].item() > 0.999 and abs(probs[0, 0, 2].sum().item() - 1) < 2e-3
    assert relerr(probs, ar.probs_ref(q.cpu(), k.cpu(), [1], B, L, Lk, Lk)) < 1e-2


# ---- 6 -------------------------------------------------------------------------------------------------------------------------
def _prepare_case(ops):
    B, L, H, Lk, kv_rows = 3, 60, 4, 1500, 1500
    q, k = _qk(B, L, H, kv_rows, seed=61, scale=1.5)
    probs = _probs(ops, q, k, [0, 1, 2, 3], B, L, Lk, kv_rows)
    return probs, [50, 37, 9], 4


@pytest.mark.parametrize("width", [1, 7, 9])
def test_align_prepare(ops, width):
    probs, n_tok, first = _prepare_case(ops)
    n_frames = [1500, 733, width // 2 if width > 1 else 2]    # the last row: no longer than the padding -> unfiltered
    B = probs.shape[0]
    nt = torch.tensor(n_tok, dtype=torch.int32, device="cuda")
    nf = torch.tensor(n_frames, dtype=torch.int32, device="cuda")
    cost = torch.full((B, probs.shape[2], 1504), 123.0, dtype=torch.float32, device="cuda")
    ops.align_prepare(probs, nt, nf, first, 1500, width, cost=cost)
    torch.cuda.synchronize()
    host = probs.cpu()
    err_k = err_r = 0.0
    for b in range(B):
        N, S = n_tok[b], n_frames[b]
        w = host[b, :, first:first + N, :S]
        r32 = ar.prepare_ref(w, width)
        r64 = ar.prepare_ref(w.double(), width)
        got = cost[b, :N, :S].cpu()
        assert torch.isfinite(got).all()
        err_k = max(err_k, (got.double() - r64).abs().max().item())
        err_r = max(err_r, (r32.double() - r64).abs().max().item())
        assert (cost[b, N:] == 123.0).all() and (cost[b, :, S:] == 123.0).all()      # only the valid block is written
    print(f"align_prepare width {width}: max abs error vs float64: kernel {err_k:.3e}, fp32 restatement {err_r:.3e}")
    assert err_k <= 4 * err_r, (err_k, err_r)


# ---- 7 -------------------------------------------------------------------------------------------------------------------------
def _dtw_check(ops, mats):
    """mats: list of numpy [N, M] fp32 -> one launch over the ragged batch, compared row by row with the reference function"""
    B = len(mats)
    L = max(m.shape[0] for m in mats)
    S = max(m.shape[1] for m in mats)
    cost = torch.full((B, L, S), float("nan"), dtype=torch.float32)
    for b, m in enumerate(mats):
        cost[b, :m.shape[0], :m.shape[1]] = torch.from_numpy(m)
    nt = torch.tensor([m.shape[0] for m in mats], dtype=torch.int32, device="cuda")
    nf = torch.tensor([m.shape[1] for m in mats], dtype=torch.int32, device="cuda")
    first = torch.full((B, L), -5, dtype=torch.int32, device="cuda")
    ops.dtw(cost.cuda(), nt, nf, S, first_frame=first)
    torch.cuda.synchronize()
    first = first.cpu()
    for b, m in enumerate(mats):
        want = ar.reference_first_frame(m)
        assert first[b, :m.shape[0]].tolist() == want.tolist(), (b, m.shape)
        assert (first[b, m.shape[0]:] == -5).all()


def test_dtw_random_shapes(ops):
    rng = np.random.default_rng(7)
    shapes = [(1, 1), (1, 1500), (5, 3), (26, 1500), (223, 1500), (447, 1500), (447, 900)]
    _dtw_check(ops, [rng.standard_normal(s).astype(np.float32) for s in shapes])


def test_dtw_ties_inf_nan(ops):
    rng = np.random.default_rng(8)
    const = np.zeros((31, 200), dtype=np.float32)
    rep = rng.standard_normal((40, 300)).astype(np.float32)
    for i in range(40):
        rep[i, 5 * i:5 * i + 6] = -1.5                          # repeated values along a diagonal band
    coarse = (np.round(rng.standard_normal((64, 500)) * 2) / 2).astype(np.float32)
    holes = rng.standard_normal((30, 250)).astype(np.float32)
    holes[7, 20:200] = np.inf
    holes[12, ::3] = -np.inf
    holes[20, 100] = np.nan
    nan = np.full((26, 1500), np.nan, dtype=np.float32)         # the degenerate case: zero spread in every column
    _dtw_check(ops, [const, rep, coarse, holes, nan])


def test_dtw_on_the_prepare_kernels_output(ops):
    probs, n_tok, first = _prepare_case(ops)
    n_frames = [1500, 733, 40]
    nt = torch.tensor(n_tok, dtype=torch.int32, device="cuda")
    nf = torch.tensor(n_frames, dtype=torch.int32, device="cuda")
    cost = ops.align_prepare(probs, nt, nf, first, 1500, 7)
    ff = ops.dtw(cost, nt, nf, 1500)
    torch.cuda.synchronize()
    host = cost.cpu().numpy()
    for b in range(len(n_tok)):
        want = ar.reference_first_frame(host[b, :n_tok[b], :n_frames[b]])
        assert ff[b, :n_tok[b]].cpu().tolist() == want.tolist(), b
        assert (ff[b, n_tok[b]:] == 0).all()


# ---- 8 / 9 ---------------------------------------------------------------------------------------------------------------------
class _Recorder:
    """Stands in for alignment.extract_token_timestamps: the same call with its intermediates kept."""

    def __init__(self, monkeypatch):
        from distil_whisper_amd import alignment
        self.calls = []
        orig = alignment.extract_token_timestamps

        def wrapped(model, sequences, enc_out, alignment_heads, num_frames=None, num_input_ids=None, time_precision=0.02):
            ts, probs, cost, first, n_tok, frames = orig(model, sequences, enc_out, alignment_heads, num_frames,
                                                         num_input_ids, time_precision, return_intermediates=True)
            self.calls.append(dict(ts=ts.cpu(), cost=None if cost is None else cost.cpu(), n_tok=n_tok, frames=frames,
                                   P=num_input_ids, probs_finite=bool(torch.isfinite(probs[..., :1500]).all())))
            return ts
        monkeypatch.setattr(alignment, "extract_token_timestamps", wrapped)

    def check_plumbing(self):
        """every call's timestamps == the reference's DTW function on the cost matrix the GPU produced"""
        assert self.calls
        for c in self.calls:
            ts, P, N = c["ts"], c["P"], c["n_tok"]
            assert c["probs_finite"] and ts.dtype == torch.float32 and not ts[:, :P].any()
            for b in range(ts.shape[0]):
                want = ar.reference_first_frame(c["cost"][b, :N, :c["frames"][b]].numpy()) * 0.02
                want = np.concatenate([want, want[-1:]]).astype(np.float32)
                assert np.array_equal(ts[b, P:].numpy(), want), (b, ts[b, P:].tolist(), want.tolist())


_share = ar.far_tokens


@pytest.mark.parametrize("graphs", [False, True])
@pytest.mark.parametrize("name", ["plain", "attention_mask", "prompt_ids", "return_timestamps", "ragged_finish"])
def test_generate_end_to_end(ops, monkeypatch, name, graphs):
    sc = SC[name]
    rec = _Recorder(monkeypatch)
    model, out = ar.run_dropin(ops, sc, META, use_graphs=graphs)
    assert out["sequences"].tolist() == sc["sequences"], name
    rec.check_plumbing()
    far, total = _share(out["token_timestamps"].cpu().tolist(), sc["token_timestamps"])
    allowed = max(2 * sc["ref_bf16_share"] * total, 1.0)
    print(f"e2e {name} graphs={graphs}: {far} of {total} tokens more than one frame from the fp32 reference "
          f"(allowed {allowed:.2f}; the reference's bf16 run: {sc['ref_bf16_share'] * total:.0f})")
    assert far <= allowed, (name, far, total, allowed)
    ts = out["token_timestamps"].cpu()
    assert (ts >= 0).all() and (ts <= 30.0).all()


def _check_segments(sc, out):
    """per segment: the window's values plus the window's offset; against the fixture as in test_generate_end_to_end"""
    from oracle import gen_golden_decode as gd
    segs, want = out["segments"][0], sc["segments"][0]
    assert out["sequences"].tolist() == sc["sequences"], sc["name"]
    assert [list(s["tokens"]) for s in segs] == [s["tokens"] for s in want]
    for s in segs:
        raw = s["result"]["token_timestamps"][s["idxs"][0]:s["idxs"][1]]
        assert len(raw) == len(s["tokens"]) == len(s["token_timestamps"])
        # The window's start in seconds (seek * 0.01, TF:800-802), read off the segment's own `start`: a segment that opens with
        # a timestamp token starts at the window's start plus that token's time (TF:2018-2025), any other at the window's start
        # (TF:2061).  The segment's values are the window's plus that offset, added as the reference adds it (a float32 row
        # plus a double scalar).
        t0 = s["tokens"][0]
        off = float(s["start"]) - ((t0 - gd.TS0) * 0.02 if t0 >= gd.TS0 else 0.0)
        assert abs(off * 100 - round(off * 100)) < 1e-6 and off >= -1e-9, off
        off = round(off * 100) / 100
        assert torch.equal(s["token_timestamps"], raw + torch.tensor(off, dtype=torch.float64)), (off, raw.tolist())
    assert max(float(s["start"]) for s in segs) >= 30.0          # the offsets matter: segments of later windows
    m = ar.segment_shares(sc, out)
    print(f"e2e {sc['name']}: {m['segment_tokens_far']} of {m['segment_tokens']} segment tokens more than one frame from the "
          f"fp32 reference (allowed {m['segment_tokens_allowed']}; the reference's bf16 run: {m['segment_tokens_far_ref_bf16']})")
    assert m["segment_tokens_far"] <= m["segment_tokens_allowed"]
    assert m["tokens_far"] <= m["tokens_allowed"]


def test_generate_seek_loop_segments(ops, monkeypatch):
    """An input longer than 30 s with return_segments=True whose tokens are pinned against bf16 noise by the generator's rule."""
    sc = SC["seek_short"]
    rec = _Recorder(monkeypatch)
    model, out = ar.run_dropin(ops, sc, META)
    assert set(out) == {"sequences", "token_timestamps", "segments"}
    rec.check_plumbing()
    assert len(rec.calls) >= 2                                  # one alignment pass per window
    _check_segments(sc, out)


def test_generate_seek_loop_45_seconds(ops, monkeypatch):
    """The 45 s scenario (some 38 windows, ~190 kept tokens): the same checks, sequences identical to the fixture included.
    The generator's token-noise rule is not applied to this scenario (tools/gen_golden_token_timestamps.py says why); that the
    MI355X path decodes the fixture's tokens is what this test asserts and profiles/token_timestamps_bench.json records."""
    sc = SC["longform_segments"]
    rec = _Recorder(monkeypatch)
    model, out = ar.run_dropin(ops, sc, META)
    rec.check_plumbing()
    assert len(rec.calls) >= 10
    _check_segments(sc, out)
