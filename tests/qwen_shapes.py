"""The cases of tests/golden/qwen_lm_shapes.npz (and the two of qwen_lm.npz): configurations, lengths, and the decode geometry each one
claims to reach.  Shared by the generator (tests/golden/make_qwen_golden.py shapes), tests/test_qwen_emo_cpu.py and the GPU tests; it
imports no transformers.

The geometry is restated here from the library's workspace layout (csrc/qwen.hip: QwenModel::carve, decode_step; csrc/qwen.h: qwen_nsplit_for;
csrc/qwen_kernels.hip: the GEMV launcher), in plain Python, so a case that stops reaching its path fails a CPU test instead of passing quietly:
    Smax      = (P + max_new + 3) & ~3           rows of the KV cache
    nsplit    = min(16, max(1, cdiv(Smax, 64)))  key pieces of a decode step (1: the unsplit return)
    slice_cap = cdiv(Smax, nsplit)               score slots of a piece; > 256 makes the 256-thread score pass loop twice
    prefill   : one piece of P score slots per query head of the group, G * P * 4 bytes of LDS (<= 40 KB)
    GEMV      : cdiv(K, 512) chunks of 512 k on the 1 / 2 / 4 / 6-chunk template
"""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass

import numpy as np

from indextts_amd import synth
from indextts_amd.qwen_emo import QwenConfig, synth_qwen_weights


def cdiv(a: int, b: int) -> int:
    return (a + b - 1) // b


def geometry(P: int, max_new: int) -> tuple:
    """(Smax, nsplit, slice_cap) of a generate(P prompt ids, max_new)."""
    smax = (P + max_new + 3) & ~3
    nsplit = min(16, max(1, cdiv(smax, 64)))
    return smax, nsplit, cdiv(smax, nsplit)


def gemv_template(K: int) -> tuple:
    """(chunks of 512 that hold some k < K, chunks of the template the launcher picks)."""
    n = cdiv(K, 512)
    return n, (1 if n <= 1 else 2 if n <= 2 else 4 if n <= 4 else 6)


def _reduced(H, I, Hq, Hkv, vocab, tied):
    return QwenConfig(vocab_size=vocab, hidden_size=H, intermediate_size=I, num_hidden_layers=2, num_attention_heads=Hq,
                      num_key_value_heads=Hkv, tie_word_embeddings=tied, max_context=512)


CONFIGS = {
    "tiny": dataclasses.replace(QwenConfig.tiny(), max_context=5120),      # G = 2; K = 128, 256; context for the longest case
    "g1": _reduced(640, 1536, 2, 2, 1000, False),           # G = 1; K = 640 (2 chunks, clamp inside chunk 1), 1536 (3 chunks on the 4 template);
                                                            # 500 row pairs = 15 workgroups of 32 + 20; lm_head.weight
    "g4": _reduced(1024, 2560, 4, 1, 512, True),            # G = 4 (6 items for 4 waves to stage); K = 2560 (5 chunks on the 6 template)
    "g3": _reduced(256, 3072, 6, 2, 512, True),             # G = 3, two kv heads; K = 768 (o_proj: 2 chunks, clamp inside chunk 1)
    "full": QwenConfig(),
}


@dataclass(frozen=True)
class Case:
    name: str
    cfg: str
    P: int
    max_new: int
    smax: int           # claimed; checked against geometry()
    nsplit: int
    slice_cap: int
    n_cols: int = 0     # stored columns (0: every column)
    file: str = "qwen_lm_shapes.npz"
    weights_tag: str = ""      # "": golden/qwen/shapes/<cfg>; the seed search is over the prompt only
    prompt_tag: str = ""       # "": golden/qwen/shapes/<name>

    def config(self) -> QwenConfig:
        return CONFIGS[self.cfg]

    def prompt(self, seed: int) -> np.ndarray:
        tag = self.prompt_tag or f"golden/qwen/shapes/{self.name}"
        return synth.integers(f"{tag}/s{seed}/prompt", (self.P,), 0, CONFIGS[self.cfg].vocab_size).astype(np.int32)


def _tiny(P, n, smax, nsplit, cap, n_cols=0, suffix=""):
    return Case(f"tiny_p{P}_n{n}{suffix}", "tiny", P, n, smax, nsplit, cap, n_cols)


SHAPE_CASES = [
    _tiny(1, 3, 4, 1, 4, 64),                    # one-row prefill, shortest cache
    _tiny(1, 200, 204, 4, 51, 64),              # pieces without a key on the first steps (n_keys < nsplit)
    _tiny(40, 25, 68, 2, 34, 64),               # first size past qwen_lm.npz's
    _tiny(40, 25, 68, 2, 34, 64, "_b"),         # a second prompt of the same shape (kept-graph reuse)
    _tiny(63, 8, 72, 2, 36, 64), _tiny(64, 8, 72, 2, 36, 64), _tiny(65, 8, 76, 2, 38, 64),          # prefill: one wave of keys
    _tiny(255, 8, 264, 5, 53, 64), _tiny(256, 8, 264, 5, 53, 64), _tiny(257, 8, 268, 5, 54, 64),    # prefill: one pass of 256 threads
    _tiny(980, 40, 1020, 16, 64, 64),           # full split
    _tiny(4200, 60, 4260, 16, 267, 64),         # a piece of 267 keys: the score pass loops twice; prefill LDS 2 * 4200 * 4 = 33.6 KB
    Case("g1", "g1", 40, 60, 100, 2, 50, 64),
    Case("g4", "g4", 40, 60, 100, 2, 50, 64),
    Case("g3", "g3", 40, 60, 100, 2, 50, 64),
    Case("full_long", "full", 150, 100, 252, 4, 63, 512, weights_tag="golden/qwen/full"),
]
LM_CASES = [      # qwen_lm.npz: weights and prompt share one searched seed
    Case("tiny", "tiny", 40, 24, 64, 1, 64, 0, "qwen_lm.npz", "golden/qwen/tiny", "golden/qwen/tiny"),
    Case("full", "full", 40, 24, 64, 1, 64, 4096, "qwen_lm.npz", "golden/qwen/full", "golden/qwen/full"),
]
BY_NAME = {c.name: c for c in SHAPE_CASES + LM_CASES}
REDUCED = [c.name for c in SHAPE_CASES if c.cfg != "full"]


def stop_step(ids):
    """The first step k >= 9 whose id has not come before and which the host's look every 8 steps does not fall on, or None."""
    ids = list(ids)
    return next((k for k in range(9, len(ids)) if (k + 1) % 8 != 0 and ids.index(ids[k]) == k), None)


def weights_tag(case: Case, fixture) -> str:
    """The synth tag of a case's weights: <tag>/s<weight seed>."""
    base = case.weights_tag or f"golden/qwen/shapes/{case.cfg}"
    return f"{base}/s{int(fixture[case.name + '_wseed'] if case.name + '_wseed' in fixture else fixture[case.name + '_seed'])}"


def case_weights(case: Case, fixture) -> dict:
    return synth_qwen_weights(case.config(), tag=weights_tag(case, fixture))


def check_claims(case: Case) -> None:
    """The case reaches what the list says it reaches."""
    cfg, G = case.config(), CONFIGS[case.cfg].num_attention_heads // CONFIGS[case.cfg].num_key_value_heads
    assert geometry(case.P, case.max_new) == (case.smax, case.nsplit, case.slice_cap), (case.name, geometry(case.P, case.max_new))
    assert case.smax <= cfg.max_context and G * cfg.max_context <= 10240 and G * case.P * 4 <= 40 * 1024, case.name
    if case.name == "tiny_p1_n200":
        assert case.P + 1 < case.nsplit                                  # steps with fewer keys than pieces
    if case.name == "tiny_p4200_n60":
        assert case.slice_cap > 256 and cdiv(case.P + 1, case.nsplit) > 256 and G * case.P * 4 == 33600
    H, I, QD, V = cfg.hidden_size, cfg.intermediate_size, cfg.num_attention_heads * 128, cfg.vocab_size
    if case.name == "g1":
        assert G == 1 and not cfg.tie_word_embeddings and gemv_template(H) == (2, 2) and 0 < H % 512 and gemv_template(I) == (3, 4)
        last = 32 * (cdiv(V // 2, 32) - 1)      # first row pair of the head's last workgroup: 4 waves of 8
        assert last + 16 < V // 2 < last + 24      # its wave 2 stops part-way, its wave 3 at once
    if case.name == "g4":
        assert G == 4 and G + 2 > 4 and gemv_template(I) == (5, 6)
    if case.name == "g3":
        assert G == 3 and cfg.num_key_value_heads == 2 and QD == 768 and gemv_template(QD) == (2, 2) and 0 < QD % 512


# ---- the three comparisons every fixture case gets (GPU tests: test_qwen_shapes_gpu.py, test_qwen_emo_gpu.py) ----
def stored(name: str, fixture) -> tuple:
    case = BY_NAME[name]
    prompt, ids = fixture[name + "_prompt"], fixture[name + "_ids"]
    assert len(prompt) == case.P and len(ids) == case.max_new
    return prompt, ids, fixture[name + "_cols"]


def check_against_reference(lm, name: str, fmt: str, fixture) -> None:
    """Teacher-forced on the stored ids: every step's logits within the case's tolerance and every step's own argmax; then the
    free-running ids."""
    prompt, ids, cols = stored(name, fixture)
    ref, tol = fixture[name + "_logits"], float(fixture[name + "_logit_tol"])
    own, lg = lm.generate(prompt, len(ids), forced_ids=ids, logits=True, logit_cols=cols)
    lg = lg.cpu().numpy()
    assert lg.shape == ref.shape
    err = np.abs(lg - ref).max(axis=1)
    print(f"{name}/{fmt}: worst |logit - reference| {err.max():.3e} (step {int(err.argmax())}) = {err.max() / tol:.3f} x logit_tol {tol:.3e} "
          f"(eps {float(fixture[name + '_eps']):.3e})")
    assert np.isfinite(lg).all() and err.max() <= tol, f"worst logit error {err.max():.3e} > logit_tol {tol:.3e}"
    assert own == ids.tolist()
    free, _ = lm.generate(prompt, len(ids))
    assert free == ids.tolist()


def check_formats_agree(lm_f32, lm_bf16, name: str, fixture) -> None:
    import torch
    prompt, ids, cols = stored(name, fixture)
    a, b = (lm.generate(prompt, len(ids), forced_ids=ids, logits=True, logit_cols=cols) for lm in (lm_f32, lm_bf16))
    assert a[0] == b[0] and torch.equal(a[1], b[1])


def check_graph_equals_eager(lm, name: str, fixture) -> None:
    import torch
    prompt, ids, cols = stored(name, fixture)
    eager = lm.generate(prompt, len(ids), logits=True, logit_cols=cols, use_graph=False)
    graph = lm.generate(prompt, len(ids), logits=True, logit_cols=cols, use_graph=True)
    assert eager[0] == graph[0] == ids.tolist() and torch.equal(eager[1], graph[1])
    assert 0 < lm.step_graph_launches() <= 5 * BY_NAME[name].config().num_hidden_layers + 3      # five launches a layer + the tail's three
