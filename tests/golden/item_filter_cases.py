"""Item-filter fixture cases shared by the generator (gen_item_filter_golden.py, runs the reference under a filtered closure) and the tests.
Inputs only: the filter lists are derived from the recorded unfiltered outputs (bssd_golden.json) and from seeds, nothing is stored as code.

On the inputs of the two strict-trie cases (600 items, 64 first-level codes):
  block_top3        exclude the three best items of the unfiltered run;
  block_first_code  exclude every item under the unfiltered best item's first code, so the closure blocks a first-level node;
  allow_pick        allow a seeded pick of 2 * DK + 5 items (never fewer allowed candidates than DK at any step: there the reference's own
                    pick among -inf ties is unspecified and its trie raises on the dead beams).
"""
from __future__ import annotations

import numpy as np

from tests.golden.cases import CASES, build_case_inputs

BASES = ("k8_dk16_trie", "k20_dk40_trie")
KINDS = ("block_top3", "block_first_code", "allow_pick")
# seed of allow_pick per base case: the first one from 0 whose run keeps every top-k margin above MIN_MARGIN and DK candidates at every step
ALLOW_SEED = {"k8_dk16_trie": 0, "k20_dk40_trie": 0}
MIN_MARGIN = 1e-4


def base_case(name):
    return next(c for c in CASES if c["name"] == name)


def filter_lists(name: str, kind: str, items, unfiltered_tokens, seed=None):
    """{"exclude": [...]} or {"allow": [...]}: lists of items' code-token sequences.  `unfiltered_tokens` = the recorded `tg_tokens` of the
    unfiltered run (best first), `items` = the case's item table."""
    items = [[int(t) for t in it] for it in items]
    if kind == "block_top3":
        return {"exclude": [[int(t) for t in row] for row in unfiltered_tokens[:3]]}
    if kind == "block_first_code":
        first = int(unfiltered_tokens[0][0])
        return {"exclude": [it for it in items if it[0] == first]}
    if kind == "allow_pick":
        case = base_case(name)
        rng = np.random.default_rng(ALLOW_SEED[name] if seed is None else seed)
        uniq = sorted({tuple(it) for it in items})
        pick = rng.choice(len(uniq), size=2 * case["DK"] + 5, replace=False)
        return {"allow": [list(uniq[i]) for i in sorted(pick)]}
    raise KeyError(kind)


def enough_candidates(allow, dk: int) -> bool:
    """at every step at least DK distinct allowed prefixes"""
    return all(len({tuple(q[:d]) for q in allow}) >= dk for d in range(1, len(allow[0]) + 1))


def all_cases():
    return [(b, k) for b in BASES for k in KINDS]


def case_id(base: str, kind: str) -> str:
    return f"{base}-{kind}"


__all__ = ["BASES", "KINDS", "ALLOW_SEED", "MIN_MARGIN", "base_case", "filter_lists", "enough_candidates", "all_cases", "case_id",
           "build_case_inputs"]
