#!/usr/bin/env python3
"""Generate tests/golden/item_filter_golden.json by RUNNING the reference (as gen_golden.py does, whose harness this reuses) with a
filtered closure (tests/item_filter_ref.closure) around the case's own trie mask: per case the BSSD result with its per-round trace and the
plain beam search of the target.  Every case also runs through the oracle with `beamsd_ref.MARGINS` installed; a case is kept only when
its smallest top-k margin is above MIN_MARGIN (fp32 noise is about 2e-5), an allow_pick case otherwise takes the next seed -- put the seed
printed here into item_filter_cases.ALLOW_SEED.

Run (CPU, about a minute):  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_item_filter_golden.py
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from tests.golden import gen_golden as G                              # noqa: E402  the reference and its harness
from atspeed_amd import synth                                         # noqa: E402
from oracle import beamsd_ref as R                                    # noqa: E402
from oracle.llama_ref import RefLlama                                 # noqa: E402
from tests import item_filter_ref as F                                # noqa: E402
from tests.golden import item_filter_cases as IC                      # noqa: E402


def run(name, kind, lists, ci, case):
    fn = F.closure(ci["fn"], synth.RESPONSE_SEP, **lists)
    target = G.HFAdapter(ci["target_dims"], ci["target_sd"], case["K"])
    draft = G.HFAdapter(ci["draft_dims"], ci["draft_sd"], case["DK"])
    inputs = {"input_ids": torch.from_numpy(ci["prompt"])[None, :]}
    rounds = []
    orig_verify, orig_draft = G.ref_beamsd.verify, G.ref_beamsd.draft_beam_search

    def draft_wrap(*a, **k):
        o = orig_draft(*a, **k)
        rounds.append({"step_len": list(o["step_len"]), "draft_ids": [x.tolist() for x in o["step_seq_tokens"]],
                       "draft_len": len(o["step_beam_indices"])})
        return o

    def verify_wrap(*a, **k):
        o = orig_verify(*a, **k)
        rounds[-1]["n_matches"] = int(o["n_matches"])
        return o

    G.ref_beamsd.verify, G.ref_beamsd.draft_beam_search = verify_wrap, draft_wrap
    try:
        out = G.ref_beamsd.BSSD(target, draft, inputs, case["gamma"], case["max_new_tokens"], prefix_allowed_tokens_fn=fn)
    finally:
        G.ref_beamsd.verify, G.ref_beamsd.draft_beam_search = orig_verify, orig_draft
    tg = G.ref_beamsd.target_generate(target, inputs, case["max_new_tokens"], prefix_allowed_tokens_fn=fn)
    P = len(ci["prompt"])
    # the oracle's margins under the same closure
    R.MARGINS = []
    try:
        rt, rd = RefLlama(ci["target_dims"], ci["target_sd"]), RefLlama(ci["draft_dims"], ci["draft_sd"])
        R.BSSD(rt, rd, ci["prompt"], case["gamma"], case["max_new_tokens"], case["K"], case["DK"], fn)
        R.target_generate(rt, ci["prompt"], case["max_new_tokens"], case["K"], fn)
        margin = float(min(R.MARGINS))
    finally:
        R.MARGINS = None
    return {"name": IC.case_id(name, kind), "base": name, "kind": kind,
            "bssd_tokens": out["beam_sequence"][:, P:].tolist(), "bssd_scores": [float(x) for x in out["beam_scores"].tolist()],
            "n_run": int(out["n_run"]), "total_accept_steps": int(out["total_accept_steps"]), "rounds": rounds,
            "tg_tokens": tg["beam_sequence"][:, P:].tolist(), "tg_scores": [float(x) for x in tg["beam_scores"].tolist()],
            "min_margin": margin}


def main():
    with open(os.path.join(HERE, "bssd_golden.json")) as f:
        base_gold = {c["name"]: c for c in json.load(f)}
    outs = []
    for name in IC.BASES:
        case = IC.base_case(name)
        ci = IC.build_case_inputs(case)
        for kind in IC.KINDS:
            seed = IC.ALLOW_SEED[name]
            while True:
                lists = IC.filter_lists(name, kind, ci["items"], base_gold[name]["tg_tokens"], seed)
                if kind == "allow_pick" and not IC.enough_candidates(lists["allow"], case["DK"]):
                    seed += 1
                    continue
                r = run(name, kind, lists, ci, case)
                if r["min_margin"] > IC.MIN_MARGIN:
                    break
                if kind != "allow_pick":
                    raise SystemExit(f"{r['name']}: smallest margin {r['min_margin']:.2e} is within fp32 noise and the case has no seed to move")
                seed += 1
            if kind == "allow_pick":
                r["seed"] = seed
            print(f"{r['name']:34s} n_run={r['n_run']} rounds={[x['n_matches'] for x in r['rounds']]} lossless={r['bssd_tokens'] == r['tg_tokens']} "
                  f"margin={r['min_margin']:.2e}" + (f" seed={seed}" if kind == "allow_pick" else ""))
            outs.append(r)
    with open(os.path.join(HERE, "item_filter_golden.json"), "w") as f:
        json.dump(outs, f)
    print("wrote", len(outs), "cases")


if __name__ == "__main__":
    main()
