"""The harness's shared-prefix rule (`run_inference(share_prefix=True)`: atspeed_amd.harness.common_prefix / cached_prefix_for) on ragged id
lists, and the front end's `prefix=` / `prefixes=` list rules; no GPU."""
import numpy as np
import pytest

from atspeed_amd.harness import MIN_SHARED_PREFIX, cached_prefix_for, common_prefix

HEAD = list(range(100, 136))                       # a 36-token template header


def _prompts(tails, head=HEAD):
    return [head + list(t) for t in tails]


def test_longest_common_prefix_of_ragged_prompts():
    ps = _prompts([[1, 2, 3, 4], [1, 2, 9], [1, 7, 7, 7, 7, 7, 7]])
    assert common_prefix(ps) == tuple(HEAD + [1])
    assert common_prefix(_prompts([[5, 6], [7, 8, 9]])) == tuple(HEAD)
    assert common_prefix([np.asarray(p) for p in ps]) == tuple(HEAD + [1])             # arrays as the harness holds them
    assert all(isinstance(t, int) for t in common_prefix([np.asarray(p) for p in ps]))
    # a difference in the very first token: nothing is shared
    assert common_prefix([[1] + HEAD, [2] + HEAD]) == ()


def test_the_cap_at_the_shortest_prompt_minus_one():
    """every user keeps one token to prefill: the row its first logits come from"""
    short = HEAD[:20]
    assert common_prefix([short, HEAD + [1, 2], HEAD + [3]]) == tuple(short[:19])
    assert common_prefix([HEAD, HEAD + [1]]) == tuple(HEAD[:35])                       # one prompt IS the shared opening
    assert common_prefix([HEAD[:9], HEAD]) == tuple(HEAD[:8])                          # cap 8 = the floor: kept
    assert common_prefix([HEAD[:8], HEAD]) == ()                                       # cap 7: below the floor


def test_the_floor_of_eight_tokens():
    assert MIN_SHARED_PREFIX == 8
    eight, seven = HEAD[:8], HEAD[:7]
    assert common_prefix([eight + [1, 2], eight + [3, 4]]) == tuple(eight)
    assert common_prefix([seven + [1, 2], seven + [3, 4]]) == ()
    assert common_prefix([seven + [1, 2], seven + [3, 4]], floor=7) == tuple(seven)
    assert common_prefix([eight + [1, 2], eight + [3, 4]], floor=9) == ()


def test_identical_prompts_and_one_user():
    p = HEAD + [1, 2, 3]
    assert common_prefix([p, p, p]) == tuple(p[:-1])                                   # all of it but the last token
    assert common_prefix([p]) == tuple(p[:-1])
    assert common_prefix([HEAD[:9]]) == tuple(HEAD[:8]) and common_prefix([HEAD[:8]]) == ()
    assert common_prefix([[7]]) == ()


def test_value_errors_of_list_lengths():
    with pytest.raises(ValueError):
        common_prefix([])
    with pytest.raises(ValueError):
        common_prefix([HEAD, []])
    # the front end: prefixes= needs one entry per user, and excludes prefix=
    from atspeed_amd.beamSD import _prefix_list
    assert _prefix_list(None, None, 3, None, None, None, [40, 41, 42], "t") is None
    assert _prefix_list(None, [None, None, None], 3, None, None, None, [40, 41, 42], "t") is None
    with pytest.raises(ValueError, match="one PromptPrefix"):
        _prefix_list(None, [None, None], 3, None, None, None, [40, 41, 42], "t")
    with pytest.raises(ValueError, match="one PromptPrefix"):
        _prefix_list(None, [], 1, None, None, None, [40], "t")
    with pytest.raises(ValueError, match="mutually exclusive"):
        _prefix_list(object(), [None], 1, None, None, None, [40], "t")
    with pytest.raises(TypeError):
        _prefix_list(None, ["not a prefix"], 1, None, None, None, [40], "t")


def test_a_batch_reuses_the_longest_built_prefix_its_prompts_open_with():
    """a split's last batch may hold one user, whose shared opening is its whole prompt: it takes the split's prefix, not one of its own"""
    header, longer = tuple(HEAD[:25]), tuple(HEAD[:30])
    assert cached_prefix_for(header, []) == header                                     # nothing built yet: build it
    assert cached_prefix_for(tuple(HEAD), [header]) == header
    assert cached_prefix_for(tuple(HEAD), [header, longer]) == longer
    assert cached_prefix_for(header, [longer]) == header                               # a longer one does not serve a shorter opening
    other = tuple([9] + HEAD[1:25])
    assert cached_prefix_for(tuple(HEAD), [other]) == tuple(HEAD)                      # another template's prefix does not serve
