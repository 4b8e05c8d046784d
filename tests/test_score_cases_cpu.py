"""CPU: tests/score_cases.py (the float64 reference of "Scoring given codes") against the committed reference fixtures, on the model of
weights.synth_gpt_weights(GPTConfig.tiny(), tag="golden/gptref"): layout "resume" on the uninterrupted run's codes against its own
step logits, layout "hf" against the first logits of the reference's continuations behind 1, 4 and 10 codes.  The fixtures tell the
two layouts apart; padding and lengths behave as the contract says."""
import numpy as np
import pytest

import score_cases as sk
from indextts_amd import weights
from indextts_amd.config import GPTConfig

FIXTURE_BOUND = 5e-5      # measured 7.3e-6 ("resume", all 10 columns) and 6.7e-6 ("hf"): the fixtures' own fp32 rounding


@pytest.fixture(scope="module")
def ref(golden_dir):
    g, p, cases = sk.golden(golden_dir)
    cfg = GPTConfig.tiny()
    return g, cfg, weights.synth_gpt_weights(cfg, tag="golden/gptref"), cases


@pytest.mark.parametrize("layout", ["resume", "hf"])
def test_reference_reproduces_the_fixtures(ref, layout):
    g, cfg, w, cases = ref
    codes, cols = cases[layout]
    lg = sk.ref_logits(w, cfg, g["prep_embeds"], g["prep_mask"], codes, layout=layout)
    assert lg.shape == (3, codes.shape[1], cfg.number_mel_codes)
    err = max(float(np.abs(lg[:, j] - want).max()) for j, want in cols.items())
    print(f"{layout}: max |dlogit| float64 reference vs fixtures = {err:.3e} (bound {FIXTURE_BOUND:.0e})")
    assert err <= FIXTURE_BOUND


def test_fixtures_tell_the_layouts_apart(ref):
    g, cfg, w, cases = ref
    codes, cols = cases["resume"]
    wrong = sk.ref_logits(w, cfg, g["prep_embeds"], g["prep_mask"], codes, layout="hf")
    assert float(np.abs(wrong[:, 0] - cols[0]).max()) <= FIXTURE_BOUND      # column 0 sees the start token alone
    for j in range(1, codes.shape[1]):
        assert float(np.abs(wrong[:, j] - cols[j]).max()) > 4.6, j


def test_padding_and_lengths(ref):
    """A shorter row's scored positions are those of the row alone (causal attention: the padding reaches none of them), and the
    log-probabilities are 0 from n_b on."""
    g, cfg, w, cases = ref
    codes, _ = cases["resume"]
    lens = [10, 4, 1]
    ragged = [list(codes[b, :lens[b]]) for b in range(3)]
    lg = sk.ref_logits(w, cfg, g["prep_embeds"], g["prep_mask"], ragged, layout="resume")
    full = sk.ref_logits(w, cfg, g["prep_embeds"], g["prep_mask"], codes, layout="resume")
    for b in range(3):
        np.testing.assert_allclose(lg[b, :lens[b]], full[b, :lens[b]], rtol=0, atol=1e-12)
    lp = sk.ref_logprobs(lg, ragged, lens)
    assert lp.shape == (3, 10) and (lp[1, 4:] == 0).all() and (lp[2, 1:] == 0).all() and (lp[0] < 0).all()
    assert abs(float(np.exp(sk.scc.ref_logprobs(lg[0, 3])).sum()) - 1.0) < 1e-12


def test_chunk_edges():
    assert [sk.chunk_edges([n]) for n in sk.ONE_ROW_LENGTHS] == [[1], [63], [64], [64, 1], [64, 64, 1]]
    assert sk.chunk_edges(sk.RAGGED_LENGTHS) == [64, 64, 64, 4]
    assert sk.chunk_edges([5] * 16) == [64, 16] and sk.chunk_edges([27] * 3) == [64, 17]
