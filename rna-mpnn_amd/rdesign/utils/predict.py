"""Directory of structures -> ``pdb_id,seq`` CSV: the role of the reference's ``main.py:17-31`` + ``rdesign/utils/predict.py:10-30``."""
from __future__ import annotations

import os
from typing import List, Tuple

from rnampnn.utils.data import bucket_batches

from .data import load_rna_dir, padded_loader


def predict(model, data_path: str, out_csv: str, batch_size: int = 32, max_rows: int = 32768) -> List[Tuple[str, str]]:
    """Read ``data_path`` (``coords/<id>.npy`` + ``seqs/<id>.fasta``), design a sequence for every structure in length-bucketed batches
    (``RNAModel.predict_sequences``: the tree read-out when one is attached, else the read-out's argmax) and write ``out_csv`` with one
    ``pdb_id,seq`` row per input in id order.  -> the rows."""
    model.eval()
    items = load_rna_dir(data_path)
    if not items:
        raise ValueError(f"no usable structure under {data_path} (coords/<id>.npy (L,7,3) + seqs/<id>.fasta)")
    batches = bucket_batches([c.shape[0] for _, c, _ in items], batch_size, max_rows, seed=0)
    seqs = {}
    for _, X, mask, lengths, idx in padded_loader(items, batches, device=model._device()):
        for i, s in zip(idx, model.predict_sequences(X, mask, lengths)):
            seqs[i] = s
    rows = [(items[i][0], seqs[i]) for i in range(len(items))]
    out_dir = os.path.dirname(os.path.abspath(out_csv))
    os.makedirs(out_dir, exist_ok=True)
    with open(out_csv, "w") as f:
        f.write("pdb_id,seq\n")
        for rid, s in rows:
            f.write(f"{rid},{s}\n")
    return rows
