"""The record of a user's options (beamSD._UserOpts: filter, adapter slot, prompt prefix), the host side: what `_user_opts` makes of an entry
point's keyword arguments, the refusals with their types, messages and order, and how `_chunked` slices the per-user arguments.  No GPU."""
import pytest
import torch

from atspeed_amd import _lib, beamSD
from atspeed_amd.generation_trie import PositionSetConstraint, SuffixTrieConstraint, Trie
from tests.test_lora_multi_cpu import SEP, _Model          # the fake models of the adapter front end's tests: adapters == {"a": 1}

INP = {"input_ids": torch.zeros(1, 9, dtype=torch.long)}
TRIE_FN = SuffixTrieConstraint(Trie([[1, 5, 6, 2]]), SEP)
POS_FN = PositionSetConstraint({0: [5], 1: [2]}, SEP)


def _opts(n, per_user=True, host=False, fn=TRIE_FN, who="x", **kw):
    return beamSD._user_opts(who, _Model(), _Model(), [INP] * n, fn, per_user, host, **kw)


def test_nobody_names_anything():
    assert _opts(1, per_user=False) is None and _opts(3) is None and _opts(0) is None
    assert _opts(2, exclude_items=[None, None], allow_items=[None, None], adapters=[None, None], prefixes=[None, None]) is None
    assert _opts(1, per_user=False, host=True) is None
    assert beamSD._UserOpts() == (None, 0, None, None) and beamSD._UserOpts().mask_args() == (None, 0)


def test_one_name_gives_every_user_a_record():
    assert _opts(3, adapters=[None, "a", None]) == [beamSD._UserOpts(), beamSD._UserOpts(slot=1), beamSD._UserOpts()]
    assert _opts(1, per_user=False, adapters="a") == [beamSD._UserOpts(slot=1)]
    got = _opts(2, exclude_items=[None, [[5, 6]]], allow_items=[[(5,)], None], adapters=["a", None])
    assert got == [beamSD._UserOpts((_lib.MASK_ALLOW, [[5]]), 1), beamSD._UserOpts((_lib.MASK_BLOCK, [[5, 6]]), 0)]
    assert _opts(1, per_user=False, exclude_items=[]) == [beamSD._UserOpts((_lib.MASK_BLOCK, []))]       # an empty block list is a filter
    with pytest.raises(AttributeError):                                                                 # a record is immutable
        got[0].slot = 2


def test_refusals_keep_their_types_and_messages():
    with pytest.raises(ValueError, match="adapters needs one name .or None. per user: 1 for 2 users"):
        _opts(2, who="BSSD_batch", adapters=["a"])
    with pytest.raises(ValueError, match="a single name for 2 users"):
        _opts(2, adapters="a")
    with pytest.raises(KeyError, match=r"'b'.*resident: \['a'\]"):
        _opts(2, adapters=["a", "b"])
    with pytest.raises(ValueError, match=r"exclude_items needs one list \(or None\) per user: 1 for 2 users"):
        _opts(2, exclude_items=[[[5]]])
    with pytest.raises(ValueError, match="mutually exclusive .user 1 has both"):
        _opts(2, exclude_items=[None, [[5]]], allow_items=[None, [[5]]])
    with pytest.raises(ValueError, match="x: exclude_items / allow_items need a SuffixTrieConstraint"):
        _opts(2, fn=POS_FN, allow_items=[None, [[5]]])
    with pytest.raises(ValueError, match="prefixes needs one PromptPrefix .or None. per user: 3 for 2 users"):
        _opts(2, prefixes=[None, None, None])
    with pytest.raises(ValueError, match="mutually exclusive"):
        _opts(1, prefix=object(), prefixes=[None])
    with pytest.raises(TypeError, match="user 1: a prefix is an atspeed_amd.PromptPrefix, not str"):
        _opts(2, prefixes=[None, "head"])


def test_a_call_that_is_wrong_twice_raises_what_it_always_raised():
    """the batch calls look at their adapters first, the one-user calls at their filter; the prefix comes last in both"""
    with pytest.raises(KeyError):
        _opts(2, adapters=["b", None], exclude_items=[[[5]]], prefixes=[None])
    with pytest.raises(ValueError, match="mutually exclusive"):
        _opts(1, per_user=False, adapters="b", exclude_items=[[5]], allow_items=[[5]])
    with pytest.raises(ValueError, match="exclude_items"):
        _opts(2, exclude_items=[[[5]]], prefixes=[None])
    with pytest.raises(ValueError, match="need a SuffixTrieConstraint"):                                 # the constraint's type before the prefix
        _opts(1, per_user=False, fn=None, exclude_items=[[5]], prefix="head")


def test_the_host_path_refuses_every_option_after_its_name_was_looked_up():
    for kw in (dict(exclude_items=[[5]]), dict(allow_items=[]), dict(adapters="a"), dict(prefix=object())):
        with pytest.raises(NotImplementedError, match="device path only"):
            _opts(1, per_user=False, host=True, fn=lambda b, s: [5], **kw)
    with pytest.raises(NotImplementedError, match="exclude_items / allow_items, adapter, prefix run on"):
        _opts(1, per_user=False, host=True, exclude_items=[[5]], adapters="a", prefix=object())
    with pytest.raises(KeyError, match="'b'"):
        _opts(1, per_user=False, host=True, adapters="b")


def test_chunks_slice_every_per_user_list_and_keep_the_users_place_in_the_whole_list(monkeypatch):
    monkeypatch.setattr(beamSD, "MAX_USERS_PER_CALL", 4)
    calls = []

    def call(chunk, **kw):
        calls.append((chunk, kw))
        return [f"out{u}" for u in chunk]

    users = list(range(10))
    per_user = dict(exclude_items=[[u] for u in users], allow_items=None, adapters=["a"] * 9 + ["b"], prefixes=None)
    sampled = (True, 1.0, 100, 0, 1.0)
    assert beamSD._chunked(call, users, sampled, per_user, prefix="shared") == [f"out{u}" for u in users]
    assert [c[0] for c in calls] == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9]]
    assert [(c[1]["_first_user"], c[1]["seed"]) for c in calls] == [(0, 100), (4, 104), (8, 108)]        # user u: stream seed + u, "user u" in a message
    assert calls[2][1] == dict(seed=108, _first_user=8, exclude_items=[[8], [9]], allow_items=None, adapters=["a", "b"], prefixes=None, prefix="shared")
    calls.clear()
    beamSD._chunked(call, users[:5], (False, 1.0, 0, 0, 1.0), dict(exclude_items=per_user["exclude_items"][:5]))      # greedy: no stream to place
    assert [c[1]["seed"] for c in calls] == [None, None] and calls[1][1] == dict(seed=None, _first_user=4, exclude_items=[[4]])
