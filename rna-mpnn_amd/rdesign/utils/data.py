"""Host-side input pipeline of the ``rdesign`` model: the reference's collate (``rdesign/utils/data.py:84-119``) on its item dicts, the
reference's data directory read into 6-atom items, and the padded / pinned / side-stream loader the trainer consumes.  The model takes the
first six backbone atoms (P, O5', C5', C4', C3', O3') and, unlike the main model's loader, keeps structures with missing atoms: a missing
atom is a zero coordinate (``nan_to_num`` in the reference's collate)."""
from __future__ import annotations

import glob
import os
from typing import List, Sequence, Tuple

import numpy as np
import torch

from rnampnn.config.glob import VOCAB
from rnampnn.utils.data import PaddedLoader, read_fasta

ATOMS = ("P", "O5'", "C5'", "C4'", "C3'", "O3'")
ALPHABET = "AUCG"
assert [VOCAB[c] for c in ALPHABET] == [0, 1, 2, 3]


def item_arrays(item) -> Tuple[str, np.ndarray, np.ndarray]:
    """One item dict of the reference's dataset ({'name', 'seq', 'coords': {atom: (L, 3)}}, ``RNADataset.__getitem__``) ->
    (name, coords (L, 6, 3) with NaN -> 0, labels (L,) int64): the tuple form ``load_rna_dir`` returns and the loader takes."""
    xyz = np.stack([np.nan_to_num(np.asarray(item["coords"][a]), nan=0.0) for a in ATOMS], axis=1)
    labels = np.array([ALPHABET.index(ch) for ch in item["seq"]], dtype=np.int64)
    if xyz.shape[0] != labels.shape[0]:
        raise ValueError(f"{item['name']}: {xyz.shape[0]} residues of coordinates for {labels.shape[0]} letters")
    return item["name"], xyz, labels


def featurize(batch: Sequence[dict]):
    """The reference collate on the same item dicts -> (X f32 (B, L, 6, 3), S int64 (B, L), mask f32 (B, L), lengths int32 ndarray (B,),
    names).  Missing atoms become 0 before anything else looks at them, so every residue of an item is valid: the mask is the prefix
    of ones of each item's length, padding is 0.  (The coordinates pass through float64 as in the reference, then round once to f32.)"""
    arrays = [item_arrays(it) for it in batch]
    lengths = np.array([len(it["seq"]) for it in batch], dtype=np.int32)
    B, L = len(batch), int(lengths.max())
    X = np.zeros((B, L, 6, 3), dtype=np.float64)
    S = np.zeros((B, L), dtype=np.int64)
    mask = np.zeros((B, L), dtype=np.float32)
    for i, (_, xyz, labels) in enumerate(arrays):
        n = int(lengths[i])
        X[i, :n], S[i, :n], mask[i, :n] = xyz, labels, 1.0
    return (torch.from_numpy(X).to(torch.float32), torch.from_numpy(S), torch.from_numpy(mask), lengths, [name for name, _, _ in arrays])


def load_rna_dir(path: str, max_len: int = 1 << 30) -> List[Tuple[str, np.ndarray, np.ndarray]]:
    """The layout the main loader reads (``coords/<id>.npy`` (L, 7, 3) + ``seqs/<id>.fasta``) -> [(id, coords f32 (L, 6, 3) with
    NaN -> 0, labels int64 (L,))] in id order.  Entries with a letter outside AUCG, a sequence length other than the residue count, no
    residues or more than ``max_len`` are dropped."""
    items = []
    for f in sorted(glob.glob(os.path.join(path, "coords", "*.npy"))):
        rid = os.path.splitext(os.path.basename(f))[0]
        fa = os.path.join(path, "seqs", rid + ".fasta")
        if not os.path.exists(fa):
            continue
        c = np.load(f, allow_pickle=False)
        seq = read_fasta(fa)
        if c.ndim != 3 or c.shape[1] < 6 or c.shape[2] != 3 or c.shape[0] != len(seq) or not 0 < c.shape[0] <= max_len:
            continue
        if any(ch not in VOCAB for ch in seq):
            continue
        xyz = np.nan_to_num(c[:, :6].astype(np.float32), nan=0.0)
        items.append((rid, np.ascontiguousarray(xyz), np.array([VOCAB[ch] for ch in seq], dtype=np.int64)))
    return items


def padded_loader(items, batches: Sequence[Sequence[int]], device=None, prefetch: int = 2) -> PaddedLoader:
    """``PaddedLoader`` in the 6-atom layout: yields (S int32 (B, T), X f32 (B, T, 6, 3), mask f32 (B, T), lengths (host list), indices)
    with the tensors on ``device`` (pinned staging, copies on a side stream; ``device=None`` keeps them on the host).  ``items``:
    (id, coords, labels) tuples or (coords, labels) pairs; coordinates with more than six atoms per residue are cut to the first six."""
    return PaddedLoader(items, batches, device=device, prefetch=prefetch, atoms=6)
