"""Drop-in surface of the reference's `code/beamSD.py` for the MI355X engine.

  BSSD(target_model, draft_model, inputs, gamma, max_new_tokens, logits_processor=None,
       prefix_allowed_tokens_fn=None) -> Dict            <- beamSD.py:458-542
  target_generate(model, inputs, max_new_tokens, logits_processor=None,
       prefix_allowed_tokens_fn=None) -> Dict            <- beamSD.py:544-595
  Timer(func="", sync_cuda=True, syn_device=0)            <- beamSD.py:12-37
  beam_sd_generate = BSSD (name used by BASELINE.json's north star)

Same positional order and the same result keys (`beam_sequence, beam_scores, n_run,
total_accept_steps, total_accept_tokens, ave_accept_tokens, draft_time_cost,
target_time_cost, verify_time_cost, time_cost`; consumed at `code/inference.py:179-187`).
The models are `HipLlama` objects; the whole loop runs in libatspeed_hip
(`atspeed_bssd_generate`) with one host read-back per verification round instead of the
reference's per-beam mask calls and `.tolist()` syncs (beamSD.py:62-64,371-372).

Mask functions that can `compile()` (PositionSetConstraint, SuffixTrieConstraint, prefix_allowed_tokens_fn(trie)) run
as a device automaton; any other callable is served by `hostmask.py` the way the reference does it (one host call per
beam per step, all arithmetic still in HIP).  `generation_config.do_sample` selects the sampling branch
(beamSD.py:65-75,293-321,332-369) with counter-based draws (`seed=` or torch's generator picks the stream) and, like the
reference's `_get_logits_warper`, honours the target config's `temperature`, `top_k` and `top_p` (per-row cutoffs computed on the device).
No mask at all (`prefix_allowed_tokens_fn=None`, legal in the reference: beamSD.py:460-481) runs on the device too: every token is a
candidate, the id filter of :80-86 is off as in the reference.  Extra `logits_processor` entries (the reference always passes None,
inference.py:175-176) are torch callables and are served by the host path: each step's log-softmax rows go through them between the
library's forward and its expand + top-K.  Sampling with a host-side mask or processors draws on the host from the device's
counter-based streams (hostmask.py): a callable wrapping a compilable constraint samples exactly what the device path samples for that seed.

`score_items` / `score_items_batch` score a given list of items instead of searching: the target's exact log-prob of each, the number a
constrained beam search would report for it (the rule of beamSD.py:58-64), from one forward in which a user's items share the rows of their
common prefixes (`atspeed_score_items`).  No reference counterpart.

`BSSDSession` is the queue form of BSSD_batch (lanes refilled at round boundaries, users submitted at any time); `BSSD_batch(..., lanes=N)`
runs a list through one.

The four entry points (BSSD, BSSD_batch, target_generate, target_generate_batch) share their scaffolding: `_mode` (models checked, sampling
mode and warpers), `_user_opts` (the users' own options, below), `_prepare` / `_setup` (prompts on the device, compiled constraints, the shared
`_DeviceFSM`, filter bitsets; one `_Decoder` per user, sampling and trace set),
`_host_call` (dispatch to hostmask.py and result conversion), `_chunked` (lists above MAX_USERS_PER_CALL) and `_one_user_call` /
`_batch_call` (buffers, argument marshalling and the library call: the one-user entry points keep their by-value launches, the batch ones
take one pointer array entry per user).  `_DeviceFSM` and `_Decoder` cache device objects per constraint and per (model pair, lane) and
hold what they were built from weakly; the objects themselves are owned by `_lib.Handle`.

Per-user options: what a user names for itself travels as ONE record, `_UserOpts(filter, slot, prefix)`, built from the public keyword
arguments by `_user_opts` (the validators `_filter_specs`, `_adapter_slots`, `_prefix_list`; None when nobody names anything) and handed on
whole: `_apply_opts` puts a record on the user's decoder inside the `try` whose `finally` takes everything off again (`_clear_opts`), a
session carries it in the submit record and the library clears the lane when the user leaves.  So between calls a cached decoder holds no
filter, slot 0 and no prefix, whatever the call did and however it ended.  A further option is a field of the record and a line in each of
`_user_opts`, `_apply_opts` and `_submit`.  The fields (include/atspeed_hip.h "item filters", "several RESIDENT adapters on one model",
"prompt prefixes"):
  filter (`exclude_items=` / `allow_items=`): token sequences -- what a beam generates after the prompt, e.g. an item's code tokens -- that
    the user must not be recommended, or the only ones it may be; they become the user's node bitset over the shared automaton
    (`_item_filters`, built on the device).  Draft and target see the same bits: BSSD under a filter is plain beam search under that filter.
  slot (`adapter=` / `adapters=`): the name of a LoRA adapter `HipLlama.add_lora` keeps on the target -> the slot in the user's segment of
    every target forward, so users of different fine-tunes share a batch or a session.
  prefix (`prefix=` / `prefixes=`): a `PromptPrefix` holds the K / V rows of a prompt opening that many users share; its rows are copied into
    the user's KV arenas and only the rest of the prompt is prefilled.  Results are those of the full-prompt call.
"""
from __future__ import annotations

import ctypes as C
import time
import weakref
from types import SimpleNamespace
from typing import Dict, NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from .generation_trie import ConstraintFSM, SuffixTrieConstraint, WholeSentenceTrieConstraint, free_constraint
from .model import HipLlama, PromptPrefix


class Timer:
    """Context manager / decorator; as a decorator it injects `result["time_cost"]`."""

    def __init__(self, func="", sync_cuda=True, syn_device=0):
        self.func = func
        self.sync_cuda = sync_cuda
        self.syn_device = syn_device

    def _sync(self):
        if self.sync_cuda and torch.cuda.is_available():
            torch.cuda.synchronize(self.syn_device)

    def __enter__(self):
        self.start = time.time()
        return self

    def __exit__(self, exc_type, exc_val, exc_tb):
        self._sync()
        self.time_cost = time.time() - self.start

    def __call__(self, func):
        def wrapper(*args, syn_device=None, **kwargs):
            if syn_device is not None:
                self.syn_device = syn_device
            self.start = time.time()
            result = func(*args, **kwargs)
            self._sync()
            self.time_cost = time.time() - self.start
            result["time_cost"] = self.time_cost
            return result
        wrapper.__name__ = getattr(func, "__name__", "wrapped")
        wrapper.__doc__ = func.__doc__
        return wrapper


# ---------------------------------------------------------------- device handles (cached)
class _DeviceFSM:
    """Device copy of a ConstraintFSM's CSR arrays (shared by every prompt; only the start node differs).  The library copies the arrays, so
    the cache refers to them WEAKLY: an entry goes when the `row_ptr` array it was built from is collected, i.e. with the last constraint
    object that holds the automaton.  The mask-free constraint is one object that lives as long as the process."""
    _cache: Dict[tuple, "_DeviceFSM"] = {}

    def __init__(self, fsm: ConstraintFSM, vocab_size: int):
        lib = _lib.load()
        if fsm.free:
            self._owner = _lib.Handle.create("atspeed_fsm_destroy", lib.atspeed_fsm_create_free, vocab_size)
        else:
            row_ptr, tok, nxt = (np.ascontiguousarray(a, np.int32) for a in (fsm.row_ptr, fsm.tok, fsm.nxt))
            self._owner = _lib.Handle.create("atspeed_fsm_destroy", lib.atspeed_fsm_create, row_ptr.ctypes.data, tok.ctypes.data,
                                             nxt.ctypes.data, fsm.n_nodes, len(tok), vocab_size)
            if fsm.id_filter is not None:
                _lib.check(lib.atspeed_fsm_set_id_filter(self._owner.ptr, int(fsm.id_filter[0]), int(fsm.id_filter[1])))
        self.handle = self._owner.ptr
        self.src = weakref.ref(fsm.row_ptr)      # an id() can be reused once its array is gone: `get` checks the identity

    @classmethod
    def get(cls, fsm: ConstraintFSM, vocab_size: int) -> "_DeviceFSM":
        key = (id(fsm.row_ptr), id(fsm.tok), vocab_size, fsm.id_filter)
        d = cls._cache.get(key)
        if d is None or d.src() is not fsm.row_ptr:
            d = cls._cache[key] = cls(fsm, vocab_size)
            weakref.finalize(fsm.row_ptr, cls._evict, key, d.src)
        return d

    @classmethod
    def _evict(cls, key: tuple, src) -> None:
        """weakref.finalize callback: the array behind `src` is gone, so is the entry built from it (not a later one under a reused id)"""
        if key in cls._cache and cls._cache[key].src is src:
            del cls._cache[key]


class _Decoder:
    """One user stream (private KV arenas + beam state) of a (target, draft) pair.  The cache refers to its models WEAKLY and
    drops a model's decoders when the model is collected, so `del model` really frees the weights and the ~0.27 GB of KV
    arenas per lane (a `--run_beam_sizes` sweep would otherwise keep every beam size's models resident)."""
    _cache: Dict[tuple, "_Decoder"] = {}
    _watched: set = set()

    def __init__(self, target: HipLlama, draft: Optional[HipLlama], max_prompt: int):
        with torch.cuda.device(target.device):
            self._owner = _lib.Handle.create("atspeed_decoder_destroy", _lib.load().atspeed_decoder_create, target._handle,
                                             draft._handle if draft is not None else None, max_prompt)
        self.handle, self.max_prompt = self._owner.ptr, max_prompt
        self.models = (weakref.ref(target), weakref.ref(draft) if draft is not None else None)
        for m in (target, draft):
            if m is not None and id(m) not in _Decoder._watched:
                _Decoder._watched.add(id(m))
                weakref.finalize(m, _evict_model, id(m))

    def serves(self, target, draft) -> bool:
        return self.models[0]() is target and (self.models[1]() if self.models[1] is not None else None) is draft

    @staticmethod
    def _key(target, draft, lane: int) -> tuple:
        return id(target), id(draft) if draft is not None else None, lane

    @classmethod
    def get(cls, target: HipLlama, draft: Optional[HipLlama], prompt_len: int, lane: int = 0) -> "_Decoder":
        """One decoder (= one user stream: private KV + activations) per (model pair, lane)."""
        key = cls._key(target, draft, lane)
        d = cls._cache.get(key)
        if d is None or d.max_prompt < prompt_len or not d.serves(target, draft):
            d = cls(target, draft, max(prompt_len, min(target.max_tokens, 512)))
            cls._cache[key] = d
        return d

    @classmethod
    def cached(cls, target: HipLlama, draft: Optional[HipLlama], lane: int = 0) -> "_Decoder":
        """The decoder an earlier call left for this (model pair, lane): what `last_trace` / `last_decisions` read."""
        d = cls._cache.get(cls._key(target, draft, lane))
        if d is None or not d.serves(target, draft):
            raise KeyError(f"no decoder of this model pair for lane {lane}: call BSSD (lane 0) or BSSD_batch with more than {lane} users "
                           "on these models first (and not release_decoders after it)")
        return d


def _evict_model(model_id: int) -> None:
    """weakref.finalize callback: the model with this id() is gone, so are the decoders that used it."""
    _Decoder._watched.discard(model_id)
    for k in [k for k in _Decoder._cache if model_id in k[:2]]:
        del _Decoder._cache[k]


def release_decoders(*models) -> int:
    """Free the cached per-user decoders (KV arenas: ~270 MB each at Llama-7B dims, 512 slots) of the given models, or all of
    them when called without arguments; returns how many were freed.  They are re-created on demand."""
    ids = {id(m) for m in models}
    keys = [k for k in _Decoder._cache if not ids or k[0] in ids or k[1] in ids]
    for k in keys:
        del _Decoder._cache[k]
    return len(keys)


# ---------------------------------------------------------------- what every entry point does around its library call
def _compile_constraint(fn, prompt):
    if fn is None:               # no mask: every token is a candidate (beamSD.py:469-478 builds an empty processor list)
        return free_constraint()
    return fn.compile(prompt)


def _host_path(logits_processor, prefix_allowed_tokens_fn) -> bool:
    """True when a step must call back into Python: extra logits processors, or a mask callable that cannot compile() itself."""
    if logits_processor is not None and len(logits_processor) != 0:
        return True
    return prefix_allowed_tokens_fn is not None and not hasattr(prefix_allowed_tokens_fn, "compile")


def _prompt_lists(prompts):
    """Token lists of all prompts with ONE device-to-host copy (a `.tolist()` per user is a synchronising copy each)."""
    if len(prompts) == 1:
        return [prompts[0].tolist()]
    flat = torch.cat([p.reshape(-1) for p in prompts]).tolist()
    out, s0 = [], 0
    for p in prompts:
        out.append(flat[s0: s0 + p.numel()])
        s0 += p.numel()
    return out


def _warpers(gc):
    """(top_k, top_p) of a generation config as the library takes them: 0 / 1.0 = off (`top_k in (None, 0)`, `top_p in (None, >= 1)`, or a
    config without the attribute, as `from_synthetic` / `from_state_dict` models have it)."""
    top_k, top_p = getattr(gc, "top_k", None), getattr(gc, "top_p", None)
    top_k = 0 if top_k is None else int(top_k)
    top_p = 1.0 if top_p is None else float(top_p)
    if top_k < 0 or top_p <= 0.0:
        raise ValueError(f"generation_config: top_k must be >= 0 and top_p in (0, 1], not {top_k} / {top_p}")
    return top_k, min(top_p, 1.0)


def min_tokens_to_keep(num_beams: int) -> int:
    """what transformers 4.41's `_get_logits_warper` hands the top-k / top-p warpers of a beam search with one eos id"""
    return 2 if int(num_beams) > 1 else 1


def _mode(seed, *models):
    """The models checked, then (do_sample, temperature, seed, top_k, top_p) of the call.  The reference samples when
    `target_model.generation_config.do_sample` is set (beamSD.py:479-481) with the warpers `_get_logits_warper` builds from that config:
    temperature, then top-k, then top-p (0 / 1.0 = off); draws there come from torch's global
    generator, here from a counter-based stream whose 32-bit seed is drawn from that generator (so `torch.manual_seed` makes a call
    repeatable) unless `seed` is given."""
    for m in models:
        if not isinstance(m, HipLlama):
            raise TypeError("models must be atspeed_amd.HipLlama (use HipLlama.from_hf(model) for an HF module)")
    gc = models[0].generation_config
    if not getattr(gc, "do_sample", False):
        return False, 1.0, 0, 0, 1.0
    if seed is None:
        seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
    temp = getattr(gc, "temperature", None)
    return (True, 1.0 if temp is None else float(temp), int(seed) & 0xFFFFFFFF) + _warpers(gc)


def _prompt_row(inputs) -> torch.Tensor:
    ids = inputs["input_ids"]
    if ids.dim() == 2:
        ids = ids[0]            # the reference reads batch row 0 only (beamSD.py:57,203,224)
    return ids


def _set_decoders(decs, mode, num_beams: int, seeds, trace=None) -> None:
    """Put decoders into a call's sampling mode (decoder i draws from stream seeds[i]), its warpers and, with `trace` not None, its decision
    trace setting.  The library is told about warpers and trace only when the setting changes."""
    lib = _lib.load()
    do, temp, _, top_k, top_p = mode
    off = (0, 1.0, 1)                                      # the one spelling of "both warpers off": a new decoder's state, every greedy call
    warp = (top_k, top_p, min_tokens_to_keep(num_beams)) if do and (top_k > 0 or top_p < 1.0) else off
    for d, seed in zip(decs, seeds):
        _lib.check(lib.atspeed_decoder_set_sampling(d.handle, 1 if do else 0, temp, int(seed) & 0xFFFFFFFF))
        if getattr(d, "warp", off) != warp:
            _lib.check(lib.atspeed_decoder_set_warpers(d.handle, *warp))
            d.warp = warp
        if trace is not None and getattr(d, "trace_on", False) != bool(trace):
            _lib.check(lib.atspeed_decoder_set_trace(d.handle, 1 if trace else 0))
            d.trace_on = bool(trace)


def _prepare(target: HipLlama, inputs_list, prefix_allowed_tokens_fn, opts, who: str, first_user: int = 0) -> SimpleNamespace:
    """What a call's users are made of, before any decoder is touched: prompts on the device, each user's compiled constraint (the mask
    functions look at the prompt -- position of "Response:", data.py:97-102 -- with one D2H copy per call, where the reference does one per beam
    per step, generation_trie.py:94, data.py:98), the ONE automaton they share (they may differ in their start node only) and the users'
    records `opts` (`_user_opts`), where a user with a filter now has its node bitset in `mask` (which keeps the library object alive as long
    as the record lives).  The lock-step calls (`_setup`), `BSSD_batch(lanes=N)` and `BSSDSession.submit` all start here."""
    dev = target.device
    prompts = [_prompt_row(inp).to(dev) for inp in inputs_list]
    fsms = [_compile_constraint(prefix_allowed_tokens_fn, ids) for ids in _prompt_lists(prompts)]
    for f in fsms[1:]:
        if f.row_ptr is not fsms[0].row_ptr:
            raise ValueError(f"{who} needs one shared constraint automaton (only the start node may differ per user)")
    dfsm = _DeviceFSM.get(fsms[0], target.dims.vocab_size)
    if opts is not None and any(o.filter is not None for o in opts):
        owners, masks = _item_filters(dfsm, [f.start for f in fsms], [o.filter for o in opts], dev, who, first_user)
        opts = [o if m is None else o._replace(mask=(next(ow for ow in owners if ow.ptr is m[0]), m[1])) for o, m in zip(opts, masks)]
    return SimpleNamespace(dev=dev, prompts=prompts, fsms=fsms, dfsm=dfsm, opts=opts)


def _setup(target: HipLlama, draft: Optional[HipLlama], inputs_list, prefix_allowed_tokens_fn, mode, who: str, opts, trace=None,
           first_user: int = 0) -> SimpleNamespace:
    """The device path's call setup, for one user or a lock-step batch: `_prepare`, then one decoder per user (lane), set to the call's
    sampling mode (user u draws from stream seed + u) and, for BSSD (`trace` not None), its decision trace.  The users' records `opts` go
    onto the decoders around the library call itself (`_apply_opts` / `_clear_opts` in `_one_user_call` and `_batch_call`)."""
    c = _prepare(target, inputs_list, prefix_allowed_tokens_fn, opts, who, first_user)
    c.bssd = draft is not None
    c.decs = [_Decoder.get(target, draft, int(p.numel()), lane=i) for i, p in enumerate(c.prompts)]
    _set_decoders(c.decs, mode, target.generation_config.num_beams, [mode[2] + u for u in range(len(c.decs))], trace)
    return c


# ---------------------------------------------------------------- per-user options: one record, one builder, one refusal, one apply, one clear
class _UserOpts(NamedTuple):
    """what one user of a call names for itself (module docstring, "Per-user options")"""
    filter: Optional[tuple] = None            # (mode, [token sequence, ...]) as `_filter_specs` makes it, None = unfiltered
    slot: int = 0                             # the target's resident adapter slot (`_adapter_slots`), 0 = none
    prefix: Optional[PromptPrefix] = None     # checked by `_prefix_list`
    mask: Optional[tuple] = None              # (owner of the call's node bitsets, the user's index in them): `_prepare` makes it of `filter`

    def mask_args(self):
        """(masks, user) as atspeed_decoder_set_node_mask and the session's submit record take them"""
        return (self.mask[0].ptr, self.mask[1]) if self.mask else (None, 0)


def _user_opts(who: str, target, draft, inputs_list, prefix_allowed_tokens_fn, per_user: bool, host: bool, exclude_items=None, allow_items=None,
               adapters=None, prefix=None, prefixes=None):
    """The public keyword arguments of an entry point -> one `_UserOpts` per user, or None when no user names anything.  `per_user`: the batch
    calls (one list entry or None per user; `prefix` = one for all), else a one-user call (`adapters` = its `adapter=`).  `host`: the call
    takes the host path, where naming any option is refused.  Every check a call makes on its options before it touches the device, in the
    order the entry points have always made them (the batch calls look at their adapters first, the one-user calls at their filter)."""
    n = len(inputs_list)
    slots = _adapter_slots(target, adapters, n, True, who) if per_user else None
    specs = _filter_specs(n, exclude_items, allow_items, per_user, who)
    if not per_user:
        slots = _adapter_slots(target, adapters, n, False, who)
    if host:
        named = [name for name, v in (("exclude_items / allow_items", specs), ("adapter", slots), ("prefix", prefix)) if v is not None]
        if named:
            raise NotImplementedError(f"{who}: {', '.join(named)} run on the device path only (a mask that can compile() itself, no extra "
                                      "logits_processor); on the host path put a filter into the mask callable and give the model its one "
                                      "adapter with load_lora")
        return None
    if specs is not None:
        _check_filter_constraint(prefix_allowed_tokens_fn, who)
    plist = _prefix_list(prefix, prefixes, n, target, draft, slots, [int(_prompt_row(inp).numel()) for inp in inputs_list], who)
    if specs is None and slots is None and plist is None:
        return None
    return [_UserOpts(specs[u] if specs else None, slots[u] if slots else 0, plist[u] if plist else None) for u in range(n)]


def _apply_opts(c: SimpleNamespace) -> None:
    """The users' records onto their decoders, every field of every user: called inside the `try` whose `finally` is `_clear_opts`.  A call
    that names nothing sets nothing: the decoders hold nothing between calls."""
    if c.opts is None:
        return
    lib = _lib.load()
    for d, o in zip(c.decs, c.opts):
        _lib.check(lib.atspeed_decoder_set_node_mask(d.handle, *o.mask_args()))
        _lib.check(lib.atspeed_decoder_set_adapter(d.handle, o.slot))
        _lib.check(lib.atspeed_decoder_set_prefix(d.handle, o.prefix.handle() if o.prefix else None,
                                                  o.prefix.handle(True) if o.prefix and c.bssd else None))


def _clear_opts(c: SimpleNamespace) -> None:
    """A cached decoder keeps nothing of a call, however the call ended: a later call that names nothing is unfiltered, runs without adapter
    and prefills its whole prompt (and the call's bitsets and prefixes may die).  Host-only calls that cannot fail."""
    if c.opts is None:
        return
    lib = _lib.load()
    for d in c.decs:
        lib.atspeed_decoder_set_node_mask(d.handle, None, 0)
        lib.atspeed_decoder_set_adapter(d.handle, 0)
        lib.atspeed_decoder_set_prefix(d.handle, None, None)


# ---------------------------------------------------------------- item filters
def _filter_specs(n: int, exclude_items, allow_items, per_user: bool, who: str):
    """One entry per user: None (unfiltered) or (mode, [token sequence, ...]).  The one-user calls take the list itself, the batch calls one
    list (or None) per user; a user has an exclude list or an allow list, never both."""
    if exclude_items is None and allow_items is None:
        return None
    if not per_user:
        if exclude_items is not None and allow_items is not None:
            raise ValueError(f"{who}: exclude_items and allow_items are mutually exclusive")
        exclude_items, allow_items = [exclude_items], [allow_items]
    specs = []
    for name, lists in (("exclude_items", exclude_items), ("allow_items", allow_items)):
        if lists is not None and len(lists) != n:
            raise ValueError(f"{who}: {name} needs one list (or None) per user: {len(lists)} for {n} users")
    for u in range(n):
        ex = exclude_items[u] if exclude_items is not None else None
        al = allow_items[u] if allow_items is not None else None
        if ex is not None and al is not None:
            raise ValueError(f"{who}: exclude_items and allow_items are mutually exclusive (user {u} has both)")
        if ex is None and al is None:
            specs.append(None)
        else:
            mode, seqs = (_lib.MASK_BLOCK, ex) if ex is not None else (_lib.MASK_ALLOW, al)
            specs.append((mode, [[int(t) for t in q] for q in seqs]))
    return specs if any(sp is not None for sp in specs) else None


def _check_filter_constraint(prefix_allowed_tokens_fn, who: str) -> None:
    """A filter's sequences are walked as items through the automaton: that needs a strict item trie (a tree below the start node)."""
    fn = prefix_allowed_tokens_fn
    if not isinstance(fn, (SuffixTrieConstraint, WholeSentenceTrieConstraint)) or fn.trie._chained():
        raise ValueError(f"{who}: exclude_items / allow_items need a SuffixTrieConstraint or an unchained WholeSentenceTrieConstraint "
                         f"(the nodes of {type(fn).__name__ if fn is not None else 'a mask-free search'}"
                         f"{' with a chained trie' if hasattr(fn, 'trie') else ''} are not items)")


def _item_filters(dfsm: _DeviceFSM, starts, specs, dev, who: str, first_user: int = 0):
    """The node bitsets of a call's filtered users -> (owners, per user None or (masks pointer, index)).  The users of one mode are built by
    ONE create call (a call whose users are all excluded-from or all allowed-to makes exactly one); `owners` keeps the library objects
    alive.  A user whose filter leaves it nothing raises ValueError before anything is launched."""
    lib = _lib.load()
    owners, per_user = [], [None] * len(specs)
    for mode in (_lib.MASK_BLOCK, _lib.MASK_ALLOW):
        users = [u for u, sp in enumerate(specs) if sp is not None and sp[0] == mode]
        if not users:
            continue
        toks, seq_off, user_off = [], [0], [0]
        for u in users:
            for q in specs[u][1]:
                toks += q
                seq_off.append(len(toks))
            user_off.append(len(seq_off) - 1)
        a_tok = np.asarray(toks if toks else [0], np.int32)
        a_soff, a_uoff = np.asarray(seq_off, np.int32), np.asarray(user_off, np.int32)
        a_start = np.asarray([starts[u] for u in users], np.int32)
        unknown, status = np.zeros(len(users), np.int32), np.zeros(len(users), np.int32)
        with torch.cuda.device(dev):
            owner = _lib.Handle.create("atspeed_node_masks_destroy", lib.atspeed_node_masks_create, dfsm.handle, len(users), a_start.ctypes.data,
                                       a_tok.ctypes.data, a_soff.ctypes.data, a_uoff.ctypes.data, mode, unknown.ctypes.data,
                                       status.ctypes.data, _lib.stream_ptr(dev))
        owners.append(owner)
        for i, u in enumerate(users):
            if status[i] != 0:
                what = ("exclude_items blocks every item the constraint allows" if mode == _lib.MASK_BLOCK
                        else f"allow_items holds no sequence the constraint knows ({int(unknown[i])} unknown)")
                raise ValueError(f"{who}: user {first_user + u}: {what}: the constraint is unsatisfiable")
            per_user[u] = (owner.ptr, i)
    return owners, per_user


# ---------------------------------------------------------------- resident adapters (HipLlama.add_lora), one per user
def _adapter_slots(target, adapters, n: int, per_user: bool, who: str):
    """The call's `adapter=` (one name or None) / `adapters=` (a list with one name or None per user) -> None when no user names an
    adapter, else the target's slot per user.  Wrong list length: ValueError; a name the target does not hold: KeyError naming the ones it does."""
    if not per_user:
        adapters = None if adapters is None else [adapters]
    if adapters is None:
        return None
    if isinstance(adapters, str) or len(adapters) != n:
        raise ValueError(f"{who}: adapters needs one name (or None) per user: "
                         f"{'a single name' if isinstance(adapters, str) else len(adapters)} for {n} users")
    if all(a is None for a in adapters):
        return None
    known = getattr(target, "adapters", {})
    for a in adapters:
        if a is not None and a not in known:
            raise KeyError(f"{who}: no resident adapter named {a!r} on the target model (HipLlama.add_lora); resident: {sorted(known)}")
    return [0 if a is None else int(known[a]) for a in adapters]


# ---------------------------------------------------------------- prompt prefixes (PromptPrefix), one per user
def _prefix_list(prefix, prefixes, n: int, target, draft, slots, prompt_lens, who: str):
    """The call's `prefix=` (one PromptPrefix for every user) / `prefixes=` (a list with one PromptPrefix or None per user) -> None when no
    user names one, else one per user.  ValueError: both given, a wrong list length, a prefix of other models (`draft` None: the target's
    half alone counts), a prefix without the draft's half in a beam-SD call, a prefix built under another adapter than the user's, a stale
    prefix, a prompt that is not longer than its prefix."""
    if prefix is not None and prefixes is not None:
        raise ValueError(f"{who}: prefix= (one for all users) and prefixes= (one per user) are mutually exclusive")
    if prefix is not None:
        prefixes = [prefix] * n
    if prefixes is None:
        return None
    if isinstance(prefixes, PromptPrefix) or len(prefixes) != n:
        raise ValueError(f"{who}: prefixes needs one PromptPrefix (or None) per user: "
                         f"{'a single object' if isinstance(prefixes, PromptPrefix) else len(prefixes)} for {n} users")
    if all(p is None for p in prefixes):
        return None
    for u, p in enumerate(prefixes):
        if p is None:
            continue
        if not isinstance(p, PromptPrefix):
            raise TypeError(f"{who}: user {u}: a prefix is an atspeed_amd.PromptPrefix, not {type(p).__name__}")
        if p.target is not target or (draft is not None and p.draft is not None and p.draft is not draft):
            raise ValueError(f"{who}: user {u}: the prompt prefix was built on other models than the call's")
        if draft is not None and p.draft is None:
            raise ValueError(f"{who}: user {u}: the prompt prefix holds the target's half alone (PromptPrefix(target, None, ...)): a beam-SD "
                             "call needs the draft's too")
        slot = slots[u] if slots is not None else 0
        if p.slot != slot:
            raise ValueError(f"{who}: user {u}: the prompt prefix was built under adapter {p.adapter!r}, the user runs under "
                             f"{'another one' if slot else 'none'}")
        if p.info()["stale"] or (draft is not None and p.info(True)["stale"]):
            raise ValueError(f"{who}: user {u}: the prompt prefix is stale (its model's quantisation or adapter changed after it was built): "
                             "build a new PromptPrefix")
        if prompt_lens is not None and p.length > prompt_lens[u] - 1:
            raise ValueError(f"{who}: user {u}: a prefix of {p.length} tokens needs a prompt of at least {p.length + 1}, got {prompt_lens[u]}")
    return list(prefixes)


def _host_call(host_fn, models, inputs: Dict, args, logits_processor, prefix_allowed_tokens_fn, mode) -> Dict:
    """Arbitrary Python callables (a mask closure, extra logits processors) are served like the reference does, one host call per beam per
    step: `host_fn(*models, prompt, *args, fn, processors, sample)` of hostmask.py, its arrays back on the device.  With do_sample the draws happen
    on the host, from the device's streams.  BSSD's statistics keys come with the result (stage times are wall clock with a device
    synchronisation, like the reference's Timer)."""
    if mode[0] and mode[1] <= 0.0:
        raise ValueError("sampling needs a temperature > 0")
    dev = models[0].device
    prompt = _prompt_row(inputs).to(dev).cpu().numpy().astype(np.int64)
    r = host_fn(*models, prompt, *args, prefix_allowed_tokens_fn, list(logits_processor or ()),
                sample=mode[1:] if mode[0] else None)
    return dict(r, beam_sequence=torch.from_numpy(r["beam_sequence"]).to(dev), beam_scores=torch.from_numpy(r["beam_scores"]).to(dev),
                n_valid=int(len(r["beam_scores"])))


def _one_user_call(entry, c: SimpleNamespace, k: int, max_new_tokens: int, *middle):
    """`entry(decoder, prompt, P, automaton, start node, *middle, tokens, scores, &stats, stream)`, the by-value launches of one user
    -> (result with `beam_sequence` [k, P + L] int64 = prompt ++ suffix per beam, stats)"""
    prompt, dev = c.prompts[0], c.dev
    with torch.cuda.device(dev):
        ids32 = prompt.to(torch.int32).contiguous()
        toks = torch.empty(k, max_new_tokens, dtype=torch.int32, device=dev)
        scores = torch.empty(k, dtype=torch.float32, device=dev)
        stats = _lib.GenStats()
        try:
            _apply_opts(c)
            _lib.check(entry(c.decs[0].handle, ids32.data_ptr(), int(prompt.numel()), c.dfsm.handle, c.fsms[0].start, *middle,
                             toks.data_ptr(), scores.data_ptr(), C.byref(stats), _lib.stream_ptr(dev)))
        finally:
            _clear_opts(c)
    seq = torch.cat((prompt.to(torch.int64)[None, :].repeat(k, 1), toks.to(torch.int64)), dim=1)
    return {"beam_sequence": seq, "beam_scores": scores}, stats


def _batch_buffers(prompts, k: int, max_new_tokens: int, dev):
    """One allocation / conversion for a whole lock-step batch instead of three small kernels per user: the prompts as ONE int32 buffer,
    the K x L token block and the K scores of every user as slices of two tensors."""
    lens = [int(p.numel()) for p in prompts]
    flat = torch.cat([p.reshape(-1) for p in prompts]).to(torch.int32)          # two kernels for the whole batch
    starts = [0]
    for n_tok in lens:
        starts.append(starts[-1] + n_tok)
    ids32 = [flat[s0: s0 + n_tok] for s0, n_tok in zip(starts, lens)]
    toks = torch.empty(len(prompts), k, max_new_tokens, dtype=torch.int32, device=dev)
    scores = torch.empty(len(prompts), k, dtype=torch.float32, device=dev)
    return ids32, toks, scores, (flat, starts)


def _batch_results(keep, toks: torch.Tensor, scores: torch.Tensor, k: int):
    """`beam_sequence` [k, P + L] int64 of every user (prompt ++ suffix per beam, beamSD.py:87,383) as views of ONE buffer written by one
    launch (atspeed_assemble_sequences) instead of a torch.cat per user."""
    flat, starts = keep
    n, L = toks.shape[0], toks.shape[2]
    off = np.asarray(starts, dtype=np.int64)
    # under the MODEL's device like every other library call: the library stages `off` through the ring of the thread's current device
    with torch.cuda.device(toks.device):
        out = torch.empty(k * (int(off[-1]) + n * L), dtype=torch.int64, device=toks.device)
        _lib.check(_lib.load().atspeed_assemble_sequences(flat.data_ptr(), off.ctypes.data, toks.data_ptr(), n, k, L, out.data_ptr(),
                                                          _lib.stream_ptr(toks.device)))
    res = []
    for i in range(n):
        o0, P = k * (int(off[i]) + i * L), int(off[i + 1] - off[i])
        res.append({"beam_sequence": out[o0: o0 + k * (P + L)].view(k, P + L), "beam_scores": scores[i]})
    return res


def _batch_call(entry, c: SimpleNamespace, k: int, max_new_tokens: int, *middle):
    """`entry(decoders, n, prompts, lengths, automaton, start nodes, *middle, tokens, scores, stats, stream)` with one pointer / int32 array
    entry per user -> (what `_batch_results` needs, stats[n]); the caller stops its clock when this returns"""
    n = len(c.prompts)
    ptrs, ints = C.c_void_p * n, C.c_int32 * n
    with torch.cuda.device(c.dev):
        ids32, toks, scores, keep = _batch_buffers(c.prompts, k, max_new_tokens, c.dev)
        stats = (_lib.GenStats * n)()
        try:
            _apply_opts(c)
            _lib.check(entry(ptrs(*[d.handle for d in c.decs]), n, ptrs(*[t.data_ptr() for t in ids32]),
                             ints(*[int(p.numel()) for p in c.prompts]), c.dfsm.handle, ints(*[f.start for f in c.fsms]), *middle,
                             ptrs(*[t.data_ptr() for t in toks]), ptrs(*[t.data_ptr() for t in scores]), stats, _lib.stream_ptr(c.dev)))
        finally:
            _clear_opts(c)
    return (keep, toks, scores, k), stats


MAX_USERS_PER_CALL = 256


def _chunked(call, inputs_list, mode, per_user: Dict, **shared):
    """The library batches up to MAX_USERS_PER_CALL users per forward; a longer list goes chunk by chunk through the entry point itself,
    `call(chunk, seed=, _first_user=, ...)`: user u of the list still draws from stream seed + u and is still user u in a message.
    `per_user`: the call's per-user keyword arguments (a list or None each), sliced like the inputs; `shared` goes to every chunk as it is."""
    outs = []
    for i in range(0, len(inputs_list), MAX_USERS_PER_CALL):
        part = slice(i, i + MAX_USERS_PER_CALL)
        outs += call(inputs_list[part], seed=(mode[2] + i) if mode[0] else None, _first_user=i,
                     **{name: None if v is None else v[part] for name, v in per_user.items()}, **shared)
    return outs


def _bssd_stats(st, k: int) -> Dict:
    """One user's BSSD statistics (beamSD.py:527-541) from the library's record of the run."""
    n_run = int(st.n_run)
    total = int(st.total_accept_steps)
    return {
        "n_run": n_run,
        "total_accept_steps": total,
        "total_accept_tokens": total * k,
        "ave_accept_tokens": total * k / n_run if n_run else 0.0,
        "draft_time_cost": st.draft_ms * 1e-3,
        "target_time_cost": st.target_ms * 1e-3,
        "verify_time_cost": st.verify_ms * 1e-3,
        "device_time_cost": st.total_ms * 1e-3,
        "accept_steps": [int(st.accept_steps[i]) for i in range(min(n_run, _lib.MAX_NEW_TOKENS))],
        "n_valid": int(st.n_valid),
        "n_target_forwards": int(st.n_target_forwards),
        "n_draft_forwards": int(st.n_draft_forwards),
        "n_target_passes": int(st.n_target_passes),
    }


# ---------------------------------------------------------------- entry points
@Timer()
@torch.no_grad()
def BSSD(target_model, draft_model, inputs: Dict, gamma: int, max_new_tokens: int,
         logits_processor=None, prefix_allowed_tokens_fn=None, seed=None, trace_decisions: bool = False,
         exclude_items=None, allow_items=None, adapter=None, prefix=None) -> Dict:
    mode = _mode(seed, target_model, draft_model)
    host = _host_path(logits_processor, prefix_allowed_tokens_fn)
    opts = _user_opts("BSSD", target_model, draft_model, [inputs], prefix_allowed_tokens_fn, False, host, exclude_items, allow_items, adapter, prefix)
    if host:
        from .hostmask import bssd_host_mask
        return _host_call(bssd_host_mask, (target_model, draft_model), inputs, (int(gamma), int(max_new_tokens)), logits_processor,
                          prefix_allowed_tokens_fn, mode)
    k = int(target_model.generation_config.num_beams)                 # beamSD.py:482
    dk = int(draft_model.generation_config.num_beams)                 # beamSD.py:483
    c = _setup(target_model, draft_model, [inputs], prefix_allowed_tokens_fn, mode, "BSSD", opts, trace_decisions)
    out, stats = _one_user_call(_lib.load().atspeed_bssd_generate, c, k, max_new_tokens, int(gamma), int(max_new_tokens), k, dk)
    out.update(_bssd_stats(stats, k))
    return out


beam_sd_generate = BSSD


class BSSDSession:
    """A queue of BSSD users over `lanes` decoders (`atspeed_session_*`): `submit(inputs)` only queues a user and returns its ticket, `step()`
    runs ONE round -- every free lane first takes the next queued user, in submission order; then the draft steps, the one target
    forward (packed, or in phases where staged verification applies: switch `verify_staged`) and the verify walks of all occupied lanes -- and returns `[(ticket, result)]` for the users that finished in it, `drain()` steps
    until queue and lanes are empty.  A user that finishes frees its lane at the next round boundary instead of waiting for the slowest user
    of its chunk, and users may be submitted while others are decoding.

    Every result equals the user's own `BSSD` call (scores to fp32 rounding, as `BSSD_batch`) and has `BSSD_batch`'s keys plus `lane`,
    `rounds_in_lane` (rounds it took part in) and `rounds_queued` (rounds the session ran while it waited); `time_cost` runs from submit to
    the step that returned it.  With `do_sample` the user of ticket t draws from stream `seed + t - 1` whichever lane it lands on (`submit`'s
    own `seed=` overrides that).

    Device path only (the rules of `_setup`): a mask callable that cannot `compile()`, extra logits processors and `trace_decisions` raise
    ValueError, and so does a user whose constraint is not the automaton of the session's first user (start nodes may differ).
    `max_prompt` (default: the decoders' usual capacity, min(max_tokens, 512)) bounds the prompts the session takes: a longer one makes
    `submit` raise AtSpeedError (ERR_CAPACITY) and leaves the session usable.  The library session is created with the first submit (the
    automaton is known then) and makes every allocation its rounds need there; `counters()` reports what ran.  The session owns its lanes'
    decoders (about 270 MB of KV memory each at the Llama-7B dims) until `close()`; it is a context manager."""

    def __init__(self, target_model, draft_model, lanes: int, gamma: int, max_new_tokens: int, prefix_allowed_tokens_fn=None,
                 max_prompt: Optional[int] = None, seed=None, logits_processor=None, trace_decisions: bool = False, _cached_decoders: bool = False):
        self.mode = _mode(seed, target_model, draft_model)
        if _host_path(logits_processor, prefix_allowed_tokens_fn):
            raise ValueError("BSSDSession runs on the device only: the mask must be able to compile() itself and there is no logits_processor")
        if trace_decisions:
            raise ValueError("BSSDSession keeps no decision trace: use BSSD / BSSD_batch with trace_decisions=True")
        if not 1 <= int(lanes) <= MAX_USERS_PER_CALL:
            raise ValueError(f"BSSDSession: lanes must be in 1 .. {MAX_USERS_PER_CALL}, not {lanes}")
        self.target, self.draft, self.fn = target_model, draft_model, prefix_allowed_tokens_fn
        self.n_lanes, self.gamma, self.max_new_tokens = int(lanes), int(gamma), int(max_new_tokens)
        self.k = int(target_model.generation_config.num_beams)
        self.dk = int(draft_model.generation_config.num_beams)
        self.max_prompt = int(max_prompt) if max_prompt is not None else min(target_model.max_tokens, 512)
        self.dev = target_model.device
        self._cached_decoders = _cached_decoders
        self._owner = self._decs = self._dfsm = self._fsm0 = None
        self._users: Dict[int, SimpleNamespace] = {}
        self._done_buf = (_lib.SessionDone * (2 * self.n_lanes))()      # a round's users, and those a failed round before it left
        self._submitted, self._closed = 0, False

    # ---- the library session, made when the first user shows which automaton the session runs on
    def _create(self, fsm: ConstraintFSM) -> None:
        lib = _lib.load()
        self._fsm0, self._dfsm = fsm, _DeviceFSM.get(fsm, self.target.dims.vocab_size)
        if self._cached_decoders:          # BSSD_batch(lanes=N): the lanes BSSD_batch itself would use
            self._decs = [_Decoder.get(self.target, self.draft, self.max_prompt, lane=i) for i in range(self.n_lanes)]
        else:
            self._decs = [_Decoder(self.target, self.draft, self.max_prompt) for _ in range(self.n_lanes)]
        _set_decoders(self._decs, self.mode, self.k, [self.mode[2]] * self.n_lanes, trace=False)    # the user's own seed comes with its admission,
        with torch.cuda.device(self.dev):                                                          # and so do its options (the library clears them when it leaves)
            self._owner = _lib.Handle.create("atspeed_session_destroy", lib.atspeed_session_create,
                                             (C.c_void_p * self.n_lanes)(*[d.handle for d in self._decs]), self.n_lanes, self._dfsm.handle,
                                             self.gamma, self.max_new_tokens, self.k, self.dk, self.max_prompt, _lib.stream_ptr(self.dev))

    def _submit(self, prompt: torch.Tensor, fsm: ConstraintFSM, ids32: torch.Tensor, toks: torch.Tensor, scores: torch.Tensor, seed=None,
                opts: _UserOpts = _UserOpts()) -> int:
        """`opts`: the user's record as `_prepare` returns it; it stays alive, its node bitset and prefix with it, until the ticket has come back"""
        if self._closed:
            raise RuntimeError("BSSDSession is closed")
        if self._fsm0 is None:
            self._create(fsm)
        elif fsm.row_ptr is not self._fsm0.row_ptr:
            raise ValueError("BSSDSession needs one shared constraint automaton (only the start node may differ per user)")
        if seed is None:
            seed = self.mode[2] + self._submitted
        user = SimpleNamespace(prompt=prompt, ids32=ids32, toks=toks, scores=scores, stats=_lib.GenStats(), t0=time.time(), opts=opts)
        ticket = C.c_int64(0)
        # host only: the library queues the user and launches nothing, so no device guard (one per user would be the call's largest cost)
        fields = (ids32.data_ptr(), int(prompt.numel()), fsm.start, int(seed) & 0xFFFFFFFF, toks.data_ptr(), scores.data_ptr(), C.pointer(user.stats),
                  *opts.mask_args(), opts.slot)
        if opts.prefix is None:            # the record without the prefix pair: the library reads the pair as NULL
            rec = _lib.SessionUser(C.sizeof(_lib.SessionUser), *fields)
        else:
            rec = _lib.SessionUserPrefix(C.sizeof(_lib.SessionUserPrefix), *fields, opts.prefix.handle(), opts.prefix.handle(True))
        _lib.check(_lib.load().atspeed_session_submit_ex(self._owner.ptr, C.byref(rec), C.byref(ticket)))
        self._submitted += 1
        self._users[ticket.value] = user
        return ticket.value

    @torch.no_grad()
    def submit(self, inputs: Dict, seed=None, exclude_items=None, allow_items=None, adapter=None, prefix=None) -> int:
        """Queue one user; no forward is launched.  Returns its ticket.  `exclude_items` / `allow_items`: the user's item filter (a list of
        token sequences; its node bitset is built here and follows the user to whichever lane it lands on).  `adapter`: the name of the
        resident adapter (`HipLlama.add_lora` on the target) the user runs under, None = none; it follows the user likewise, and must stay
        resident until the user's ticket has come back.  `prefix`: the `PromptPrefix` the user's prompt opens with; the session keeps it
        alive until the ticket has come back."""
        opts = _user_opts("BSSDSession.submit", self.target, self.draft, [inputs], self.fn, False, False, exclude_items, allow_items, adapter, prefix)
        c = _prepare(self.target, [inputs], self.fn, opts, "BSSDSession.submit", self._submitted)
        prompt = c.prompts[0]
        with torch.cuda.device(self.dev):
            ids32 = prompt.to(torch.int32).contiguous()
            toks = torch.empty(self.k, self.max_new_tokens, dtype=torch.int32, device=self.dev)
            scores = torch.empty(self.k, dtype=torch.float32, device=self.dev)
        return self._submit(prompt, c.fsms[0], ids32, toks, scores, seed, c.opts[0] if c.opts else _UserOpts())

    def _finished(self, buf, n: int, assemble: bool):
        out, now = [], time.time()
        for rec in buf[:n]:
            u = self._users.pop(int(rec.ticket))
            r = {"beam_scores": u.scores}
            if assemble:
                r["beam_sequence"] = torch.cat((u.prompt.to(torch.int64)[None, :].repeat(self.k, 1), u.toks.to(torch.int64)), dim=1)
            r.update(_bssd_stats(u.stats, self.k))
            r.update({"status": int(rec.status), "time_cost": now - u.t0, "lane": int(rec.lane),
                      "rounds_in_lane": int(rec.rounds_in_lane), "rounds_queued": int(rec.rounds_queued)})
            out.append((int(rec.ticket), r))
        return out

    @torch.no_grad()
    def step(self, _assemble: bool = True):
        """Admission, one round, retirement: [(ticket, result)] of the users that finished.  Nothing queued and no lane occupied: []."""
        if self._owner is None or self._owner.ptr is None:
            return []
        return self._run(_lib.load().atspeed_session_round, self._done_buf, _assemble)

    def _run(self, call, buf, assemble: bool):
        """`call` = atspeed_session_round / _drain with room for len(buf) records.  A round that fails raises here; the users it held come
        back from the next step() / drain() with the error as their `status` (no valid beams), the queued ones are decoded as usual."""
        n = C.c_int32(0)
        with torch.cuda.device(self.dev):
            _lib.check(call(self._owner.ptr, buf, len(buf), C.byref(n)))
        return self._finished(buf, n.value, assemble)

    @torch.no_grad()
    def drain(self, _assemble: bool = True):
        """Rounds until the queue and the lanes are empty (`atspeed_session_drain`): [(ticket, result)] in the order the users finished."""
        if self._owner is None or self._owner.ptr is None or not self._users:
            return []
        return self._run(_lib.load().atspeed_session_drain, (_lib.SessionDone * len(self._users))(), _assemble)

    def counters(self) -> Dict:
        """What the session ran so far (`atspeed_session_counters`); before the first submit everything is 0."""
        c = _lib.SessionCounters()
        if self._owner is not None and self._owner.ptr is not None:
            _lib.check(_lib.load().atspeed_session_get_counters(self._owner.ptr, C.byref(c)))
        return {name: int(getattr(c, name)) for name, _ in _lib.SessionCounters._fields_}

    def close(self) -> None:
        """Destroy the library session, then the lanes it owns.  Users still queued or in lanes get no result."""
        self._closed = True
        if self._owner is not None:
            self._owner.close()
        self._users.clear()
        self._decs = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def _bssd_batch_lanes(target_model, draft_model, inputs_list, gamma, max_new_tokens, prefix_allowed_tokens_fn, seed, lanes: int, opts=None):
    """`BSSD_batch(..., lanes=N)`: the whole list through one session of N lanes, results in list order.  The prompts, token blocks and
    scores are the batch call's buffers (one allocation each) and the result tensors come from its one assemble launch; the whole list's
    filter bitsets are built up front (`_prepare`) and live in the users' records until the drain is over."""
    if not inputs_list:
        return []
    t0 = time.time()
    c = _prepare(target_model, inputs_list, prefix_allowed_tokens_fn, opts, "BSSD_batch")
    dev, prompts = c.dev, c.prompts
    n_lanes = max(1, min(int(lanes), len(prompts), MAX_USERS_PER_CALL))
    with BSSDSession(target_model, draft_model, n_lanes, gamma, max_new_tokens, prefix_allowed_tokens_fn,
                     max_prompt=max(int(p.numel()) for p in prompts), seed=seed, _cached_decoders=True) as ses:
        k = ses.k
        with torch.cuda.device(dev):
            ids32, toks, scores, keep = _batch_buffers(prompts, k, int(max_new_tokens), dev)
        tickets = [ses._submit(p, f, i32, toks[u], scores[u], opts=c.opts[u] if c.opts else _UserOpts())
                   for u, (p, f, i32) in enumerate(zip(prompts, c.fsms, ids32))]
        done = dict(ses.drain(_assemble=False))
        wall = time.time() - t0
        outs = _batch_results(keep, toks, scores, k)
        for out, t in zip(outs, tickets):
            out.update({key: v for key, v in done[t].items() if key != "beam_scores"})
            out["time_cost"] = wall / len(outs)
        outs[0]["session_counters"] = ses.counters()
    return outs


@torch.no_grad()
def BSSD_batch(target_model, draft_model, inputs_list, gamma: int, max_new_tokens: int,
               prefix_allowed_tokens_fn=None, seed=None, trace_decisions: bool = False, lanes: Optional[int] = None,
               exclude_items=None, allow_items=None, _first_user: int = 0, adapters=None, prefix=None, prefixes=None):
    """BSSD for several independent users at once (one result dict per user, same keys as BSSD).

    The reference decodes users strictly one after another (inference.py:162-176).  Here the users advance in
    lock step: each has its own decoder (private KV caches and beam state) and every draft step / target
    verification of a round is ONE forward over the tokens of all users (`atspeed_bssd_generate_batch`), so the
    weights are streamed once per forward instead of once per user.  Token ids, n_matches and draft candidates
    are identical to calling BSSD() per user (scores agree to fp32 rounding: the GEMM tiling depends on the batch).

    `lanes=N` (default None: the lock-step path above, unchanged) runs the list through a `BSSDSession` of N lanes instead: user u + N starts
    as soon as one of the first N finishes, not when all of them have.  Same results and keys (plus the session's `lane`, `rounds_in_lane`,
    `rounds_queued`; the first result also carries `session_counters`), user u still draws from stream seed + u.  One difference: a session
    refuses a prompt at submit when its rounds COULD run out of KV slots (prompt length + (max_new_tokens - 1) x draft beams > max_slots,
    AtSpeedError ERR_CAPACITY, nothing decoded), where the lock-step path only fails if that user's acceptance really takes it there.

    `exclude_items` / `allow_items`: one list of token sequences (or None = unfiltered) per user, on either path; a user has one or the other.
    `adapters`: one resident adapter's name (`HipLlama.add_lora`) or None per user, on either path: every user of the batch runs the target
    under its own adapter, the draft is never adapted.
    `prefix` (one `PromptPrefix` for every user) / `prefixes` (one or None per user), on either path: the users' shared prompt openings,
    whose K / V are copied into the users' arenas instead of being prefilled."""
    opts = _user_opts("BSSD_batch", target_model, draft_model, inputs_list, prefix_allowed_tokens_fn, True, False, exclude_items, allow_items,
                      adapters, prefix, prefixes)
    if lanes is not None:
        if trace_decisions:
            raise ValueError("BSSD_batch(lanes=N) keeps no decision trace")
        return _bssd_batch_lanes(target_model, draft_model, inputs_list, gamma, max_new_tokens, prefix_allowed_tokens_fn, seed, lanes, opts)
    mode = _mode(seed, target_model, draft_model)
    if len(inputs_list) > MAX_USERS_PER_CALL:          # the whole list's options are checked by now; every chunk builds the records of its own users
        return _chunked(lambda chunk, **kw: BSSD_batch(target_model, draft_model, chunk, gamma, max_new_tokens, prefix_allowed_tokens_fn,
                                                       trace_decisions=trace_decisions, **kw), inputs_list, mode,
                        dict(exclude_items=exclude_items, allow_items=allow_items, adapters=adapters, prefixes=prefixes), prefix=prefix)
    k = int(target_model.generation_config.num_beams)
    dk = int(draft_model.generation_config.num_beams)
    t0 = time.time()
    c = _setup(target_model, draft_model, inputs_list, prefix_allowed_tokens_fn, mode, "BSSD_batch", opts, trace_decisions, _first_user)
    raw, stats = _batch_call(_lib.load().atspeed_bssd_generate_batch, c, k, max_new_tokens, int(gamma), int(max_new_tokens), k, dk)
    wall = time.time() - t0
    outs = _batch_results(*raw)
    for out, st in zip(outs, stats):
        out.update(_bssd_stats(st, k))
        out.update({"time_cost": wall / len(outs), "status": int(st.status)})
    return outs


@Timer()
@torch.no_grad()
def target_generate(model, inputs: Dict, max_new_tokens: int, logits_processor=None,
                    prefix_allowed_tokens_fn=None, seed=None, exclude_items=None, allow_items=None, adapter=None, prefix=None) -> Dict:
    mode = _mode(seed, model)
    host = _host_path(logits_processor, prefix_allowed_tokens_fn)
    opts = _user_opts("target_generate", model, None, [inputs], prefix_allowed_tokens_fn, False, host, exclude_items, allow_items, adapter, prefix)
    if host:
        from .hostmask import target_generate_host_mask
        return _host_call(target_generate_host_mask, (model,), inputs, (int(max_new_tokens),), logits_processor, prefix_allowed_tokens_fn,
                          mode)
    k = int(model.generation_config.num_beams)                        # beamSD.py:553
    c = _setup(model, None, [inputs], prefix_allowed_tokens_fn, mode, "target_generate", opts)
    out, stats = _one_user_call(_lib.load().atspeed_target_generate, c, k, max_new_tokens, int(max_new_tokens), k)
    out.update({"n_valid": int(stats.n_valid), "device_time_cost": stats.total_ms * 1e-3})
    return out


def target_generate_batch(model, inputs_list, max_new_tokens: int, prefix_allowed_tokens_fn=None, seed=None, exclude_items=None,
                          allow_items=None, _first_user: int = 0, adapters=None, prefix=None, prefixes=None):
    """`target_generate` for several independent users in lock step (one result dict per user): position g of every
    user's constrained beam search is ONE forward.  This is the loop `code/generate_teacher_data.py:211-244` runs over
    a whole training set with HF `generate`; token ids equal per-user `target_generate` calls.  `exclude_items` / `allow_items`: one list of
    token sequences (or None = unfiltered) per user.  `adapters`: one resident adapter's name (`HipLlama.add_lora`) or None per user.
    `prefix` (one `PromptPrefix` for every user) / `prefixes` (one or None per user): the users' shared prompt openings."""
    mode = _mode(seed, model)
    opts = _user_opts("target_generate_batch", model, None, inputs_list, prefix_allowed_tokens_fn, True, False, exclude_items, allow_items,
                      adapters, prefix, prefixes)
    if len(inputs_list) > MAX_USERS_PER_CALL:
        return _chunked(lambda chunk, **kw: target_generate_batch(model, chunk, max_new_tokens, prefix_allowed_tokens_fn, **kw), inputs_list, mode,
                        dict(exclude_items=exclude_items, allow_items=allow_items, adapters=adapters, prefixes=prefixes), prefix=prefix)
    k = int(model.generation_config.num_beams)
    t0 = time.time()
    c = _setup(model, None, inputs_list, prefix_allowed_tokens_fn, mode, "target_generate_batch", opts, first_user=_first_user)
    raw, stats = _batch_call(_lib.load().atspeed_target_generate_batch, c, k, max_new_tokens, int(max_new_tokens), k)
    wall = time.time() - t0
    outs = _batch_results(*raw)
    for out, st in zip(outs, stats):
        out.update({"n_valid": int(st.n_valid), "status": int(st.status), "device_time_cost": st.total_ms * 1e-3,
                    "time_cost": wall / len(outs)})
    return outs


# ---------------------------------------------------------------- scoring candidates
def _tree_rows_added(prev, seq) -> int:
    """Tree rows sequence `seq` adds behind `prev` (None: first of its chunk) in the packed layout of include/atspeed_hip.h "scoring
    candidates": e = min(lcp, len(prev) - 1) leading depths are shared, its last token needs no row."""
    e = 0
    if prev is not None:
        lim = min(len(prev), len(seq))
        while e < lim and prev[e] == seq[e]:
            e += 1
        e = max(0, min(e, len(prev) - 1))
    return max(0, len(seq) - 1 - e)


def _score_chunks(seqs, P: int, model: HipLlama, who: str, user: int):
    """A user's sorted item list cut into runs that each fit the model with the prompt repeated in front: prompt + tree rows within
    max_tokens and max_slots, the rows from the prompt's last on within max_logit_rows.  A single item that does not fit raises."""
    cap = min(model.max_tokens, model.max_slots, model.max_logit_rows + P - 1)
    chunks, cur, rows = [], [], P
    for q in seqs:
        add = _tree_rows_added(cur[-1] if cur else None, q)
        if cur and rows + add > cap:
            chunks.append(cur)
            cur, rows = [], P
            add = _tree_rows_added(None, q)
        if rows + add > cap:
            raise ValueError(f"{who}: user {user}: a prompt of {P} tokens and one item of {len(q)} need {rows + add} rows, the model holds "
                             f"{cap} (max_tokens {model.max_tokens}, max_slots {model.max_slots}, max_logit_rows {model.max_logit_rows})")
        cur.append(q)
        rows += add
    chunks.append(cur)
    return chunks


@torch.no_grad()
def score_items_batch(model, inputs_list, items_list, prefix_allowed_tokens_fn, adapters=None, prefix=None, errors: str = "raise",
                      return_unknown: bool = False):
    """The target's exact log-prob of every listed item, per user: one fp32 tensor [len(items)] per user, in the caller's order.  An item's
    score is what a constrained beam search reports for it (the sum over its tokens of logit - LSE over the full vocabulary, in token order),
    from ONE forward over all users in which a user's items share the rows of their common prefixes.

    `items_list`: per user a list of token sequences in the form `allow_items=` takes, in any order, repeats allowed.  Items the
    constraint does not know score -inf.  `adapters`: one resident adapter's name (`HipLlama.add_lora`) or None per user.  A list that does
    not fit the model's capacity in one segment is scored in several, each repeating the prompt.
    `errors="return"`: a user that cannot be scored (a single item that does not fit behind its prompt) gets its ValueError in place of its
    tensor and the others are scored; "raise" (default) raises it.  `return_unknown`: also return the unknown items counted per user."""
    who = "score_items_batch"
    if prefix is not None:
        raise NotImplementedError(f"{who}: prompt prefixes (PromptPrefix) serve the generate calls only; the branch-scoring forward "
                                  "prefills every prompt whole")
    if errors not in ("raise", "return"):
        raise ValueError(f"{who}: errors must be 'raise' or 'return', not {errors!r}")
    _mode(None, model)
    n = len(inputs_list)
    if len(items_list) != n:
        raise ValueError(f"{who}: items_list needs one list per user: {len(items_list)} for {n} users")
    if prefix_allowed_tokens_fn is None or _host_path(None, prefix_allowed_tokens_fn):
        raise NotImplementedError(f"{who}: items are scored on the device path only (a mask that can compile() itself); "
                                  f"{type(prefix_allowed_tokens_fn).__name__ if prefix_allowed_tokens_fn is not None else 'a mask-free search'} "
                                  "has no automaton to walk them through")
    slots = _adapter_slots(model, adapters, n, True, who)
    lists = []
    for u, items in enumerate(items_list):
        seqs = [tuple(int(t) for t in q) for q in items]
        if not seqs:
            raise ValueError(f"{who}: user {u}: the item list is empty")
        for q in seqs:
            if not 1 <= len(q) <= _lib.MAX_NEW_TOKENS:
                raise ValueError(f"{who}: user {u}: an item holds 1 .. {_lib.MAX_NEW_TOKENS} tokens, not {len(q)}")
        lists.append(seqs)
    c = _prepare(model, inputs_list, prefix_allowed_tokens_fn, None, who)
    if c.fsms[0].free:
        raise NotImplementedError(f"{who}: a mask-free search has no automaton to walk the items through")
    dev, lib = c.dev, _lib.load()
    # per user: sorted, de-duplicated, cut into segments; a segment is one "user" of the library call
    segs, failed, uniq = [], {}, []
    for u, seqs in enumerate(lists):
        order = sorted(set(seqs))
        uniq.append(order)
        try:
            chunks = _score_chunks(order, int(c.prompts[u].numel()), model, who, u)
        except ValueError as e:
            if errors == "raise":
                raise
            failed[u] = e
            continue
        segs += [(u, ch) for ch in chunks]
    scores = {u: [] for u in range(n)}
    unknown = [0] * n
    with torch.cuda.device(dev):
        flat = torch.cat([p.reshape(-1) for p in c.prompts]).to(torch.int32)
        starts = np.concatenate([[0], np.cumsum([int(p.numel()) for p in c.prompts])])
        for g0 in range(0, len(segs), MAX_USERS_PER_CALL):
            part = segs[g0: g0 + MAX_USERS_PER_CALL]
            m = len(part)
            toks = np.asarray([t for _, ch in part for q in ch for t in q], np.int32)
            seq_off = np.concatenate([[0], np.cumsum([len(q) for _, ch in part for q in ch])]).astype(np.int32)
            user_off = np.concatenate([[0], np.cumsum([len(ch) for _, ch in part])]).astype(np.int32)
            a_prompt = (C.c_void_p * m)(*[flat.data_ptr() + 4 * int(starts[u]) for u, _ in part])
            a_len = np.asarray([int(c.prompts[u].numel()) for u, _ in part], np.int32)
            a_start = np.asarray([c.fsms[u].start for u, _ in part], np.int32)
            a_slot = np.asarray([slots[u] if slots else 0 for u, _ in part], np.int32)
            out = torch.empty(int(user_off[-1]), dtype=torch.float32, device=dev)
            unk, status = np.zeros(m, np.int32), np.zeros(m, np.int32)
            _lib.check(lib.atspeed_score_items(model._handle, c.dfsm.handle, m, a_prompt, a_len.ctypes.data, a_start.ctypes.data, toks.ctypes.data,
                                               seq_off.ctypes.data, user_off.ctypes.data, a_slot.ctypes.data if slots else None, out.data_ptr(),
                                               unk.ctypes.data, status.ctypes.data, _lib.stream_ptr(dev)))
            for i, (u, _) in enumerate(part):
                if status[i] != 0:           # the front end sorts and sizes the lists itself: the library disagreeing is a bug, not a user error
                    raise _lib.AtSpeedError(int(status[i]), f"{who}: user {u}: the library refused a segment the front end built")
                scores[u].append(out[int(user_off[i]): int(user_off[i + 1])])
                unknown[u] += int(unk[i])
    res = []
    for u in range(n):
        if u in failed:
            res.append(failed[u])
            continue
        s = torch.cat(scores[u]) if len(scores[u]) > 1 else scores[u][0]
        where = {q: i for i, q in enumerate(uniq[u])}
        res.append(s[torch.tensor([where[q] for q in lists[u]], device=dev)])      # the caller's order, repeats included
    return (res, unknown) if return_unknown else res


@torch.no_grad()
def score_items(model, inputs: Dict, items, prefix_allowed_tokens_fn, adapter=None, prefix=None, return_unknown: bool = False):
    """`score_items_batch` for one user: fp32 [len(items)], the target's log-prob of each item in the caller's order."""
    if prefix is not None:
        raise NotImplementedError("score_items: prompt prefixes (PromptPrefix) serve the generate calls only; the branch-scoring forward "
                                  "prefills every prompt whole")
    out = score_items_batch(model, [inputs], [items], prefix_allowed_tokens_fn, adapters=None if adapter is None else [adapter],
                            return_unknown=return_unknown)
    return (out[0][0], out[1][0]) if return_unknown else out[0]


def last_trace(target_model, draft_model):
    """Per-round trace of the last BSSD call on this model pair (parity tests):
    list of dict(draft_len, n_matches, n_beams, draft_ids=[draft_len][dk])."""
    lib = _lib.load()
    dec = _Decoder.cached(target_model, draft_model)
    n = lib.atspeed_decoder_trace(dec.handle, None, 0)
    buf = (C.c_int32 * max(n, 1))()
    lib.atspeed_decoder_trace(dec.handle, buf, n)
    dk = int(draft_model.generation_config.num_beams)
    rounds, i = [], 0
    while i < n:
        dl, nm, nb = buf[i], buf[i + 1], buf[i + 2]
        i += 3
        ids = [[int(buf[i + s * dk + j]) for j in range(dk)] for s in range(dl)]
        i += dl * dk
        rounds.append(dict(draft_len=int(dl), n_matches=int(nm), n_beams=int(nb), draft_ids=ids))
    return rounds


def last_decisions(target_model, draft_model, lane: int = 0):
    """Decision trace of the last BSSD / BSSD_batch call made with `trace_decisions=True` for the user in `lane`
    (`atspeed_decoder_decisions`): one dict per round with the beams the round started from, the draft's blocks, the target's picks of
    every verify step (the decisions of beamSD.py:297-298,323-328) and n_matches; a final single step (beamSD.py:505-509) is a round
    of kind "final".  Sequences are the generated suffixes (lists of token ids), scores fp32."""
    lib = _lib.load()
    dec = _Decoder.cached(target_model, draft_model, lane)
    n = int(lib.atspeed_decoder_decisions(dec.handle, None, 0))
    buf = np.zeros(max(n, 1), dtype=np.int32)
    lib.atspeed_decoder_decisions(dec.handle, buf.ctypes.data, n)
    B, L, G1 = _lib.MAX_BEAMS, _lib.MAX_NEW_TOKENS, _lib.MAX_GAMMA + 1
    bw = 5 * B + B * L

    def block(words, n_valid, seq_len):
        sc = words[:B].view(np.float32)
        parent, tok, flat = words[2 * B: 3 * B], words[3 * B: 4 * B], words[4 * B: 5 * B]
        seq = words[5 * B:].reshape(B, L)
        rows = [j for j in range(n_valid) if flat[j] >= 0]
        return dict(score=[float(sc[j]) for j in rows], seq=[[int(t) for t in seq[j, :seq_len]] for j in rows],
                    parent=[int(parent[j]) for j in rows], tok=[int(tok[j]) for j in rows], index=rows)

    rounds, i = [], 0
    while i < n:
        kind, nb, dl, nm, gen0, k, dk, nblk = (int(x) for x in buf[i: i + 8])
        i += 8
        blocks = [buf[i + b * bw: i + (b + 1) * bw] for b in range(nblk)]
        i += nblk * bw
        if kind == 1:
            rounds.append(dict(kind="final", gen0=gen0, k=k, parents=block(blocks[0], nb, gen0), result=block(blocks[1], k, gen0 + 1)))
            continue
        vt = buf[i: i + G1 * 3 * B].reshape(G1, 3, B)
        i += G1 * 3 * B
        start = block(blocks[0], nb, gen0)
        draft = [block(blocks[s], dk, gen0 + s) for s in range(1, dl + 1)]
        picks = []
        for s in range(nm + 1):
            src_full = blocks[s][5 * B:].reshape(B, L)
            sc, par, tok = vt[s, 0].view(np.float32), vt[s, 1], vt[s, 2]
            rows = [j for j in range(k) if tok[j] >= 0]
            picks.append(dict(score=[float(sc[j]) for j in rows], parent=[int(par[j]) for j in rows], tok=[int(tok[j]) for j in rows],
                              seq=[[int(t) for t in src_full[par[j], :gen0 + s]] + [int(tok[j])] for j in rows]))
        rounds.append(dict(kind="verify", gen0=gen0, k=k, dk=dk, draft_len=dl, n_matches=nm, start=start, draft=draft, picks=picks,
                           result=block(blocks[dl + 1], k, gen0 + nm + 1)))
    return rounds
