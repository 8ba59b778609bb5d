"""The real Beauty / Games data of the reference, as far as the harness tests read it, stored under tests/golden/ so that those
tests run wherever the repository is checked out.

`real_<name>.json.xz` holds, per dataset: the full item index (`<name>.LCRec-1e-3lr.json`) and, for every user with test items,
in the order of the reference's `testing_dict.npy`, the test items, the validation items and the last 20 training items (the test
split keeps `(train + valid)[-max_his_len:]` with max_his_len 20, so older training items never reach a prompt).  Users without
test items are dropped: `SeqRecDataset(mode="test")` skips them.

`materialize(dst)` writes them back in the reference's file formats (`<name>/<name>.LCRec-1e-3lr.json` and the three `*_dict.npy`)
so that the tests go through the same loaders (`ItemIndex.load`, `load_interactions`, `SeqRecTestData.load`) as on the original
files.  Regenerate with `python tests/golden/real_data.py <reference data dir>`.
"""
from __future__ import annotations

import json
import lzma
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DATASETS = ("beauty", "games")
INDEX_FILE = ".LCRec-1e-3lr.json"
MAX_HIS_LEN = 20


def fixture_path(name: str) -> str:
    return os.path.join(HERE, f"real_{name}.json.xz")


def materialize(dst: str) -> str:
    """Write both datasets under `dst` in the reference's layout; returns `dst` (the `data_path` the loaders take)."""
    for name in DATASETS:
        with lzma.open(fixture_path(name), "rt") as f:
            fx = json.load(f)
        d = os.path.join(dst, name)
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, name + INDEX_FILE), "w") as f:
            json.dump(fx["index"], f)
        for key, fname in (("train", "training_dict.npy"), ("valid", "validation_dict.npy"), ("test", "testing_dict.npy")):
            np.save(os.path.join(d, fname), np.array({int(u): v for u, v in fx[key]}, dtype=object), allow_pickle=True)
    return dst


def generate(src: str) -> None:
    """Build the fixtures from the reference's data directory `src` (holding beauty/ and games/)."""
    for name in DATASETS:
        d = os.path.join(src, name)
        with open(os.path.join(d, name + INDEX_FILE)) as f:
            index = json.load(f)
        tr, va, te = (np.load(os.path.join(d, f"{k}_dict.npy"), allow_pickle=True).item() for k in ("training", "validation", "testing"))
        keep = [int(u) for u in te if len(te[u])]
        fx = dict(index=index,
                  train=[[u, [int(x) for x in tr[u]][-MAX_HIS_LEN:]] for u in keep if u in tr],
                  valid=[[u, [int(x) for x in va[u]]] for u in keep if u in va],
                  test=[[u, [int(x) for x in te[u]]] for u in keep])
        with lzma.open(fixture_path(name), "wt", preset=9 | lzma.PRESET_EXTREME) as f:
            json.dump(fx, f, separators=(",", ":"))
        print(name, len(keep), "test users ->", os.path.relpath(fixture_path(name)), os.path.getsize(fixture_path(name)), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit("usage: python tests/golden/real_data.py <reference data dir holding beauty/ and games/>")
    generate(sys.argv[1])
