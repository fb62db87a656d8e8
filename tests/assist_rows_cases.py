"""TEST INFRASTRUCTURE -- inputs of the per-row acceptance tests (tests/test_assist_rows*.py).

1. Planted rounds with rows at different lengths (`make_rows_case`): one planted single-row case of tests/assist_cases.py per row,
   each with its own history length, put side by side in one token buffer of `total` columns.  What a scenario plants per row --
   the rejected position, the timestamp state, a finished row, EOS inside the drafts, min_new_tokens -- is that module's; the
   expected integers come from tests/assist_rows_restatement.py.

2. A model pair whose agreement depends on the ROW (`planted_pair`).  Seeded random weights have nearly flat logits (exact ties in
   most inputs, see tests/test_assist_gpu.py), and planting the target's sequence in the position rows alone makes every row agree
   alike.  So two things are planted, both as dual vectors W of the planted tokens' embedding rows E (W[s] . E[s'] = 1 if s == s'
   else 0, so planted columns do not leak into each other):
     * position row P - 1 + i = c_i W[seq[i]]: the logit of seq[i] at the step that emits generated token i is c_i -- 100 at a
       strong step, 50 at a `weak` one;
     * row b's encoder output is g_b W[u_b] at every source position, and the LAST decoder layer's cross-attention has v_proj = I,
       out_proj = s I (biases 0): whatever the attention weights, it adds s g_b W[u_b] to the stream, so the logit of u_b is s g_b
       at every step.  s g_b = 15 / 35 / 75 in the target and 1.8 times that (27 / 63 / 135) in the assistant, whose only
       difference from the target is that factor.
   Row 0: both models emit seq everywhere (every draft accepted).  Row 1: the assistant drafts u_1 at the weak steps (63 > 50) where
   the target keeps seq (35 < 50): rejected there.  Row 2: the target itself takes u_2 at the weak steps (75 > 50) -- with u_2 =
   EOS the row ends at the first weak step --, the assistant drafts u_2 everywhere (135 > 100): rejected at every strong step,
   accepted at the weak ones.  Every decision is at least 25 % of the best score away from turning (a bf16 ulp is under 0.8 %);
   the non-planted columns stay below 0.09 x 3.3 x |planted| ~ 36 at d_model 128 and far lower at 1280.  `scale` multiplies all of
   it (the layers' outputs are larger at d_model 1280)."""
import numpy as np
import torch

from tests import assist_cases as ac

ROW_SG = (15.0, 35.0, 75.0)                                # s g_b of the target, rows 0 / 1 / 2
ASSISTANT_FACTOR = 1.8
STRONG, WEAK, S_OUT = 100.0, 50.0, 100.0


def make_rows_case(seed, V, lens, k, name, total=None, P0=3):
    """-> dict(logits f64 [B, k + 1, V], tokens int64 [B, total], lens, k, total, P0, done, eos, fill, min_new, suppress, ts, own
    (expected, from the single-row cases), lay).  `lens`: the rows' lengths (all P0 for a scenario of the first generated position).
    total defaults to max(lens) + k + 1: the longest row reaches it when all its drafts are accepted."""
    B = len(lens)
    sc = ac.scenarios(B, k)[name]
    if sc["first"]:
        lens = [P0] * B
    total = max(lens) + k + 1 if total is None else total
    min_new = None if sc["min_new_in"] is None else (lens[0] - P0) + sc["min_new_in"]      # one threshold for the whole batch
    rows = []
    for b, L in enumerate(lens):
        one = dict(sc, reject=[sc["reject"][b]], done=[sc["done"][b]])
        if min_new is not None:
            one["min_new_in"] = min_new - (L - P0)             # (make_case adds the row's own L - P0 back)
        rows.append(ac.make_case(seed + 7919 * b, V, 1, k, one, n_hist=L - P0, P0=P0, pad_behind=0))
    c0 = rows[0]
    assert all(r["L"] == L for r, L in zip(rows, lens))
    assert all(r["min_new"] == c0["min_new"] and r["eos"] == c0["eos"] and r["ts"] == c0["ts"] for r in rows)
    tokens = np.full((B, total), 7, dtype=np.int64)            # 7: a sentinel text id behind the round
    for b, r in enumerate(rows):
        tokens[b, :r["tokens"].shape[1]] = r["tokens"][0]
    return dict(logits=np.concatenate([r["logits"] for r in rows], 0), tokens=tokens, lens=list(lens), k=k, total=total, P0=P0,
                done=np.array(sc["done"], dtype=bool), eos=c0["eos"], fill=c0["fill"], min_new=c0["min_new"],
                suppress=sorted({s for r in rows for s in r["suppress"]}), ts=c0["ts"],
                own=np.concatenate([r["own"] for r in rows], 0), lay=c0["lay"])


def planted_rows(V, lens, k, name, total=None):
    """The case of scenario `name` (first seed whose mass-rule margins are clear: assist_cases asserts it)."""
    for seed in range(40):
        try:
            return make_rows_case(1000 * seed + 17 * len(lens) + k + len(name), V, lens, k, name, total)
        except AssertionError:
            continue
    raise AssertionError(f"no clear-margin case for {name}")


def planted_pair(sd, P, seq, weak, row_tokens, d_model, max_src, scale=1.0, last_layer=None, head_gain=1.0):
    """-> (target state dict, assistant state dict, enc f32 [B * max_src, d_model]) as the module docstring describes.  sd: the
    target's seeded weights; P: decoder prompt length; seq: the planted generated tokens; weak: the indices into seq planted at
    WEAK; row_tokens: u_b per row (B <= 3); last_layer: index of the last decoder layer (default: the highest in sd).  head_gain
    multiplies the tied embedding first: behind the final LayerNorm a logit cannot exceed sqrt(d_model) |E row|, 6.4 with the
    fixture's embeddings -- the softmax is then so flat that the mass of the ~90 timestamp columns passes the best planted text
    score and the timestamp rules decide by noise; at four times the embedding the planted scores stand at ~20 against a mass
    of ~7.  Pass scale = head_gain with it: the dual vectors shrink by the gain, so the planted stream vectors -- and with them
    their size against the layers' outputs -- stay what they are at gain 1."""
    sd = dict(sd)
    sd["model.decoder.embed_tokens.weight"] = sd["model.decoder.embed_tokens.weight"] * head_gain
    E = sd["model.decoder.embed_tokens.weight"].double()
    planted = sorted(set(seq) | set(row_tokens))
    Es = E[planted]
    W = torch.linalg.solve(Es @ Es.T, Es)                      # dual vectors: W @ Es.T = I
    dual = {t: W[i] for i, t in enumerate(planted)}
    tgt = dict(sd)
    pos = sd["model.decoder.embed_positions.weight"].clone()
    for i, t in enumerate(seq):
        pos[P - 1 + i] = ((WEAK if i in weak else STRONG) * scale * dual[t]).to(pos.dtype)
    tgt["model.decoder.embed_positions.weight"] = pos
    if last_layer is None:
        last_layer = max(int(k.split(".")[3]) for k in sd if k.startswith("model.decoder.layers."))
    p = f"model.decoder.layers.{last_layer}.encoder_attn"
    eye = torch.eye(d_model, dtype=sd[f"{p}.v_proj.weight"].dtype)
    tgt[f"{p}.v_proj.weight"], tgt[f"{p}.v_proj.bias"] = eye.clone(), torch.zeros(d_model)
    tgt[f"{p}.out_proj.weight"], tgt[f"{p}.out_proj.bias"] = S_OUT * eye, torch.zeros(d_model)
    ast = dict(tgt)
    ast[f"{p}.out_proj.weight"] = ASSISTANT_FACTOR * S_OUT * eye
    rows = [(ROW_SG[b] * scale / S_OUT * dual[u]).float() for b, u in enumerate(row_tokens)]
    enc = torch.stack(rows)[:, None, :].expand(-1, max_src, -1).reshape(len(rows) * max_src, d_model).contiguous()
    return tgt, ast, enc


def expected_rows(seq, weak, row_tokens, eos, max_new):
    """What the target emits per row under `planted_pair` with no rule in the way: seq, with u_2 at the weak steps of row 2; a row
    ends behind its EOS."""
    out = []
    for b, u in enumerate(row_tokens):
        row = [u if (b == 2 and i in weak) else t for i, t in enumerate(seq[:max_new])]
        if eos is not None and eos in row:
            row = row[:row.index(eos) + 1]
        out.append(row)
    return out
