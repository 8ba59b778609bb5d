"""Sampling-mode warpers, CPU side: the cutoff rule of tests/warp_ref.py (what the device kernel and its tests restate) keeps exactly the
entries the installed transformers' TopKLogitsWarper -> TopPLogitsWarper keep, on rows whose boundaries are unambiguous; and the front end
reads `top_k` / `top_p` from the generation config the way the reference's `_get_logits_warper` does."""
from types import SimpleNamespace

import numpy as np
import pytest

from tests import warp_ref as W

SIZES = (1, 2, 3, 50, 51, 257, 4099)
TOP_KS = (1, 2, 50, 0)
TOP_PS = (0.1, 0.9, 1.0)
MARGIN = 1e-4


def _row(n, top_k, top_p, min_keep, scale=2.0, **kw):
    """the first seed whose row is unambiguous at both boundaries (margins checked, never the outcome).  A flat row of thousands of entries
    has cumulative probabilities closer than 1e-4 to one another, so some lies within 1e-4 of ANY boundary: such a shape gets peakier
    logits until a seed qualifies."""
    for sc in (scale, 2 * scale, 4 * scale, 8 * scale, 16 * scale):
        for seed in range(40):
            row = W.score_row(n, 1000 * n + seed, scale=sc, **kw)
            gk, gp = W.margins(row, top_k, top_p, min_keep, tie_at_k=bool(kw.get("tie_at")))
            if gk >= MARGIN and gp >= MARGIN:
                return row
    raise AssertionError(f"no unambiguous row of {n} entries for top_k={top_k} top_p={top_p}")


@pytest.mark.parametrize("min_keep", [1, 2])
@pytest.mark.parametrize("n", SIZES)
def test_cutoff_rule_keeps_what_the_hf_warpers_keep(n, min_keep):
    for top_k in TOP_KS:
        for top_p in TOP_PS:
            for scale, temperature, n_masked in ((2.0, 1.0, 0), (0.5, 1.3, 0), (3.0, 0.7, n // 3)):
                row = _row(n, top_k, top_p, min_keep, scale=scale, temperature=temperature, n_masked=n_masked)
                got, want = W.survivors(row, top_k, top_p, min_keep), W.hf_survivors(row, top_k, top_p, min_keep)
                assert np.array_equal(got, want), (n, top_k, top_p, min_keep, n_masked, int(got.sum()), int(want.sum()))
                if top_k == 0 and top_p >= 1.0:
                    assert W.cutoff(row, top_k, top_p, min_keep) == -np.inf and got.sum() == np.isfinite(row).sum()
                if top_k and top_p >= 1.0:
                    assert got.sum() == min(max(top_k, min_keep), np.isfinite(row).sum())


@pytest.mark.parametrize("n,top_k", [(3, 2), (51, 50), (257, 2), (4099, 50)])
def test_an_exact_tie_at_the_kth_value_survives(n, top_k):
    row = _row(n, top_k, 1.0, 2, tie_at=max(top_k, 2))
    got = W.survivors(row, top_k, 1.0, 2)
    assert got.sum() == max(top_k, 2) + 1                                  # both tied entries stay
    assert np.array_equal(got, W.hf_survivors(row, top_k, 1.0, 2))


def test_all_masked_and_short_rows():
    assert W.cutoff(np.full(7, -np.inf, np.float32), 2, 0.5, 2) == -np.inf
    row = np.asarray([-0.5, -np.inf, -2.0], np.float32)
    assert W.cutoff(row, 50, 1.0, 2) == -np.inf                           # fewer finite entries than k': the k'-th largest is -inf
    assert np.array_equal(W.survivors(row, 50, 1.0, 2), W.hf_survivors(row, 50, 1.0, 2))
    assert np.array_equal(W.survivors(row, 1, 0.1, 2), [True, False, True])   # min_keep = 2 outlives top_k = 1 and a tiny nucleus


def test_front_end_reads_the_warpers_like_get_logits_warper():
    from atspeed_amd import beamSD
    gc = SimpleNamespace(do_sample=True, temperature=0.7)
    assert beamSD._warpers(gc) == (0, 1.0)                                  # from_synthetic / from_state_dict configs: no attribute = off
    for top_k, top_p, want in ((None, None, (0, 1.0)), (0, 1.0, (0, 1.0)), (50, 1.0, (50, 1.0)), (8, 0.9, (8, 0.9)), (0, 1.5, (0, 1.0))):
        gc.top_k, gc.top_p = top_k, top_p
        assert beamSD._warpers(gc) == want
    gc.top_k = -1
    with pytest.raises(ValueError):
        beamSD._warpers(gc)
    assert beamSD.min_tokens_to_keep(1) == 1 and beamSD.min_tokens_to_keep(20) == 2
    from atspeed_amd.model import _gen_config
    assert not hasattr(_gen_config(4), "top_k") and not hasattr(_gen_config(4), "top_p")


def test_host_path_builds_the_hf_warpers_in_the_reference_order():
    from atspeed_amd import hostmask
    assert hostmask._hf_warpers(0, 1.0, 2) == []
    ws = hostmask._hf_warpers(8, 0.9, 2)
    assert [type(w).__name__ for w in ws] == ["TopKLogitsWarper", "TopPLogitsWarper"]
    assert ws[0].top_k == 8 and ws[1].min_tokens_to_keep == 2
    assert [type(w).__name__ for w in hostmask._hf_warpers(0, 0.5, 1)] == ["TopPLogitsWarper"]
    kw = hostmask._sampling_kw(None, (), (1.3, 5), 10)                      # the two-field form: no warpers
    assert kw["warpers"] == [] and kw["temperature"] == 1.3
    assert len(hostmask._sampling_kw(None, (), (1.3, 5, 50, 1.0), 10)["warpers"]) == 1


def test_inference_cli_takes_the_warpers_only_with_its_sampling_flag():
    from atspeed_amd import inference
    a = inference.parse(["--data_path", "x", "--do_sample", "--top_k", "8", "--top_p", "0.9"])
    assert a.do_sample and a.top_k == 8 and a.top_p == 0.9
    assert inference.parse(["--data_path", "x"]).top_k is None
    with pytest.raises(SystemExit):
        inference.parse(["--data_path", "x", "--top_k", "8"])
