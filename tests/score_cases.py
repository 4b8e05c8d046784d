"""Scoring given codes (include/idxtts.h "Scoring given codes"): the float64 reference of the teacher-forced log-probabilities, the
golden configuration the tests share, and the lengths that make every chunk edge of the head occur.  No GPU here:
tests/test_score_cases_cpu.py checks this file against the committed reference fixtures, the tests/test_score_*_gpu.py files check
the native call against it."""
import os

import numpy as np
import torch

import scores_cases as scc
from oracle import gpt as og

CHUNK = 64                                   # scored positions per head launch (GPTModel::SCORE_CHUNK)
POS0 = {"resume": 2, "hf": 1}
ONE_ROW_LENGTHS = (1, 63, 64, 65, 129)       # below, at and past one chunk; past two
RAGGED_LENGTHS = (1, 65, 130)                # 196 positions: three full chunks and a remainder of 4
LOGIT_BOUND = 5e-4                           # tests/test_prefix_ref_gpu.py: the same prefill against the same reference


def widen(w: dict) -> dict:
    return {k: (v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v))).to(torch.float64) for k, v in w.items()}


def input_rows(w64: dict, cfg, prompt_emb, codes, lens, layout: str) -> torch.Tensor:
    """[B, P + n, d] float64: [prompt | mel_emb[start] + mel_pos[0] | mel_emb[c_j] + mel_pos[pos0 + j], j < n_b - 1], right-padded with
    code 0 (a valid table row) up to n - 1 fed codes."""
    me, mp = w64["mel_embedding.weight"], w64["mel_pos_embedding.emb.weight"]
    emb = torch.as_tensor(np.asarray(prompt_emb)).to(torch.float64)
    B, n = len(lens), int(max(lens))
    pos0 = POS0[layout]
    rows = []
    for b in range(B):
        fed = [0] * (n - 1)
        for j in range(int(lens[b]) - 1):
            fed[j] = int(codes[b][j])
        tail = [me[cfg.start_mel_token] + mp[0]] + [me[c] + mp[pos0 + j] for j, c in enumerate(fed)]
        rows.append(torch.cat([emb[b], torch.stack(tail)]))
    return torch.stack(rows)


def ref_logits(w: dict, cfg, prompt_emb, mask, codes, lens=None, layout: str = "resume") -> np.ndarray:
    """float64 logits [B, n, V] of the scored positions P .. P + n - 1 (the fp32 model, widened exactly, every operation in double);
    mask [B, P + 1] or None: the left padding."""
    codes = [list(map(int, r)) for r in np.asarray(codes).tolist()] if not isinstance(codes, list) else codes
    lens = [len(r) for r in codes] if lens is None else [int(x) for x in lens]
    w64 = widen(w)
    x = input_rows(w64, cfg, prompt_emb, codes, lens, layout)
    B, S, _ = x.shape
    n = int(max(lens))
    P = S - n
    valid = torch.ones(B, S, dtype=torch.long)
    if mask is not None:
        valid[:, :P] = torch.as_tensor(np.asarray(mask))[:, :P]
    hidden, _ = og.gpt2_stack(w64, cfg, x, valid)
    return og.lm_head(w64, cfg, hidden[:, P:]).numpy()


def ref_logprobs(logits, codes, lens) -> np.ndarray:
    """float64 [B, n]: log-softmax of each scored position's logits at the row's code, 0 from n_b on."""
    lg = np.asarray(logits)
    B, n, _ = lg.shape
    out = np.zeros((B, n), np.float64)
    for b in range(B):
        for j in range(int(lens[b])):
            out[b, j] = scc.ref_logprobs(lg[b, j])[int(codes[b][j])]
    return out


def golden(golden_dir):
    """(gpt_ref.npz, prefix_ref.npz, {layout: (codes [3, n], {column: fixture logits [3, V]})}): "resume" = the uninterrupted run's
    10 codes against its own step logits; "hf" = those 10 and the first code the reference drew behind them, columns 1, 4 and 10
    against the first logits of its continuations behind 1, 4 and 10 codes."""
    g = np.load(os.path.join(golden_dir, "gpt_ref.npz"))
    p = np.load(os.path.join(golden_dir, "prefix_ref.npz"))
    c = g["step_codes"]
    resume = (c, {j: g["step_logits"][:, j] for j in range(c.shape[1])})
    hf = (np.concatenate([c, p["prefix_k10_codes"][:, :1]], 1), {k: p[f"prefix_k{k}_logits"][:, 0] for k in (1, 4, 10)})
    return g, p, {"resume": resume, "hf": hf}


def chunk_edges(lens) -> list:
    """Rows of every head launch of a call with these lengths."""
    T = int(sum(lens))
    return [min(CHUNK, T - c) for c in range(0, T, CHUNK)]
