"""n-best beam fixtures for tests/test_takes_gpu.py -> takes_ref.npz.

Same source as gpt_ref.npz's beam cases (make_golden.py::make_gpt_ref, f2): the reference's GPT2InferenceModel driven through the
vendored `_beam_search` loop (make_golden.drive_vendored_beam_search, imported unchanged) and the reference's own vendored
BeamSearchScorer -- here built with num_beam_hyps_to_keep = n, which is what HF's generate passes for num_return_sequences = n
(transformers_generation_utils.py:2226-2255).  Recorded per case: the stop bias, warpers, the Exp(1) draws torch.multinomial consumed,
and what finalize returned: `sequences` [B * n, L] (stop-padded) and `sequences_scores` [B * n].  Conditioning and texts are
gpt_ref.npz's (`conds`, `text`), so the file holds results only.

Run on the CPU:  python tests/golden/make_takes_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (puts the repository and the package on sys.path)

NEW, SEED = 16, 4321
# (num_beams, stop bias, temperature, top_k, top_p): a wide nucleus so that beam-sample really samples, a stop bias under which some
# hypotheses finish before the cap and others are topped up from the open beams at it
CASES = ((2, 4.0, 1.6, 30, 0.97), (3, 4.0, 1.6, 30, 0.97), (8, 4.5, 1.6, 30, 0.97))


class _KeepN:
    """Stands where drive_vendored_beam_search expects the scorer module: the reference's BeamSearchScorer, built with
    num_beam_hyps_to_keep = n, whose finalize() result is kept whole (the driver returns `sequences` only)."""

    def __init__(self, mod, n):
        self.mod, self.n, self.result = mod, n, None

    def BeamSearchScorer(self, **kw):
        kw["num_beam_hyps_to_keep"] = self.n
        scorer = self.mod.BeamSearchScorer(**kw)
        finalize = scorer.finalize

        def keep(*a, **k):
            self.result = finalize(*a, **k)
            return self.result
        scorer.finalize = keep
        return scorer


def main():
    from indextts_amd import weights
    from indextts_amd.config import GPTConfig
    mv = mg._import_reference_model_v2()
    scorer_mod = mg._import_reference_beam_scorer()
    cfg = GPTConfig.tiny()
    g = np.load(os.path.join(HERE, "gpt_ref.npz"))
    conds, text = torch.from_numpy(g["conds"]), torch.from_numpy(g["text"])
    B, V = text.shape[0], cfg.number_mel_codes
    w = weights.synth_gpt_weights(cfg, tag="golden/gptref")
    w.update(weights.synth_gpt_cond_weights(cfg, tag="golden/gptref"))
    out, ties = {"cases": np.array([c[0] for c in CASES])}, 0
    for nb, stop_bias, temperature, top_k, top_p in CASES:
        wb = dict(w)
        wb["mel_head.bias"] = w["mel_head.bias"].copy()
        wb["mel_head.bias"][cfg.stop_mel_token] += stop_bias
        uv = mg.build_reference_unified_voice(mv, cfg, wb)
        out[f"nb{nb}_stop_bias"] = np.array(stop_bias, dtype=np.float32)
        out[f"nb{nb}_warpers"] = np.array([temperature, top_k, top_p], dtype=np.float64)
        torch.manual_seed(SEED)
        out[f"nb{nb}_noise"] = torch.stack([torch.empty(B, nb * V).exponential_(1) for _ in range(NEW)]).numpy()
        for mode, do_sample in (("det", False), ("sample", True)):
            for n in sorted({1, 2, nb}):
                keep = _KeepN(scorer_mod, n)
                torch.manual_seed(SEED)
                seq = mg.drive_vendored_beam_search(uv, keep, cfg, conds, text, NEW, nb, do_sample, temperature, top_k, top_p, 10.0, 0.0)
                scores = keep.result["sequence_scores"]
                assert seq.shape[0] == B * n and scores.shape == (B * n,)
                out[f"nb{nb}_{mode}_n{n}_codes"] = seq.numpy()
                out[f"nb{nb}_{mode}_n{n}_scores"] = scores.numpy().astype(np.float32)
                sc = scores.view(B, n)
                ties += int((sc[:, 1:] == sc[:, :-1]).sum()) if n == nb else 0
                print(f"num_beams {nb} {mode} n {n}:", seq.tolist(), scores.tolist())
    print("pairs of neighbouring hypotheses with equal scores:", ties)
    np.savez_compressed(os.path.join(HERE, "takes_ref.npz"), **out)
    print("wrote takes_ref.npz", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
