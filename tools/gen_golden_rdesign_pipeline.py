#!/usr/bin/env python3
"""Generate tests/golden/rdesign_pipeline/featurize.npz: inputs and outputs of the REFERENCE's own collate, `rdesign.utils.data.featurize`
(sibling of tools/gen_golden_rdesign.py, whose import helper - real imports first, inert placeholders for absent packages, a check that no
placeholder was used - it reuses).  Build container only: needs the reference checkout; never run on the GPU box or from a test.

Inputs: seven structures of tests/data/c3_subset.npz, the first in file order of each length in LENGTHS, first six atoms, as the item
dicts `RNADataset.__getitem__` hands to the collate.  The subset holds no NaN, so missing atoms are injected by this rule:
  * item 2: residue 5 loses all six atoms;
  * item 3: residue 0 loses its P (an incomplete first residue);
  * items 4..6: every atom is dropped with probability 0.03, drawn from numpy.random.RandomState(NAN_SEED) in item order, one
    `random_sample((L, 6))` per item.
The fixture lives in a SUB-directory: every *.npz directly under tests/golden/ is enumerated by existing parametrised tests.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_rdesign_pipeline.py [--check]

`--check` regenerates into memory and compares every array with the committed fixture instead of writing.  Data only.
"""
from __future__ import annotations

import io
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden_rdesign as G                  # noqa: E402  (imports the reference's featurize on import)

REPO = G.REPO
OUT = os.path.join(REPO, "tests", "golden", "rdesign_pipeline", "featurize.npz")
LENGTHS = (114, 2, 13, 36, 160, 1, 75)          # collate order: not sorted, so padding differs per row
NAN_SEED, NAN_P = 20, 0.03
ATOMS = ["P", "O5'", "C5'", "C4'", "C3'", "O3'"]


def inputs():
    z = np.load(os.path.join(REPO, "tests", "data", "c3_subset.npz"), allow_pickle=False)
    ids = [str(i) for i in z["ids"]]
    rng = np.random.RandomState(NAN_SEED)
    names, seqs, coords = [], [], []
    for k, n in enumerate(LENGTHS):
        rid = next(i for i in ids if z["coords/" + i].shape[0] == n)
        c = np.array(z["coords/" + rid][:, :6], dtype=np.float32)
        assert not np.isnan(c).any()
        if k == 2:
            c[5] = np.nan
        elif k == 3:
            c[0, 0] = np.nan
        elif k >= 4:
            c[rng.random_sample((n, 6)) < NAN_P] = np.nan
        names.append(rid); seqs.append(str(z["seq/" + rid])); coords.append(c)
    assert sum(int(np.isnan(c).any()) for c in coords) >= 4
    return names, seqs, coords


def main():
    check = "--check" in sys.argv
    names, seqs, coords = inputs()
    batch = [{"name": n, "seq": s, "coords": {a: c[:, i, :] for i, a in enumerate(ATOMS)}} for n, s, c in zip(names, seqs, coords)]
    X, S, mask, lengths, out_names = G.featurize(batch)
    assert not G.STUB_USES, f"a placeholder import was used by the collate: {G.STUB_USES}"
    assert X.dtype == torch.float32 and S.dtype == torch.int64 and mask.dtype == torch.float32 and lengths.dtype == np.int32
    res = dict(names=np.array(names), seqs=np.array(seqs), X=X.numpy(), S=S.numpy(), mask=mask.numpy(), lengths=lengths,
               out_names=np.array(out_names))
    res.update({f"coords.{k}": c for k, c in enumerate(coords)})
    if check:
        old = np.load(OUT, allow_pickle=False)
        assert sorted(old.files) == sorted(res), "keys differ"
        for k in res:
            a, b = np.asarray(res[k]), old[k]
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"array {k} is not byte-identical"
        print(f"{len(res)} arrays byte-identical to the committed fixture ({os.path.getsize(OUT) / 1024:.0f} KB)")
        return
    buf = io.BytesIO()
    np.savez_compressed(buf, **res)
    assert buf.getbuffer().nbytes <= G.MAX_FIXTURE_BYTES
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "wb") as f:
        f.write(buf.getvalue())
    print(f"-> {OUT[len(REPO) + 1:]} {buf.getbuffer().nbytes / 1024:.0f} KB; B,L={tuple(mask.shape)} lengths {lengths.tolist()} "
          f"NaN atoms per item {[int(np.isnan(c).any(-1).sum()) for c in coords]} stubbed={G.STUBBED}")


if __name__ == "__main__":
    main()
