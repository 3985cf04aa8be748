#!/usr/bin/env python3
"""Design sequences for a directory of structures with a trained model - the role of the reference's ``main.py:17-31``:

    python rna-mpnn_amd/predict.py --ckpt runs/rnampnn/Final.pt [--xgb runs/rnampnn/XGB.json] --data /path/to/data --out submit.csv
    python rna-mpnn_amd/predict.py --ckpt runs/rnampnn/Final.pt --data /path/to/data --samples 8 --temperature 0.1 --designs-out designs.csv

``--ckpt`` is what ``train.py --out DIR`` wrote (weights + constructor arguments, loaded with ``weights_only=True``; pickles are never
loaded).  Its ``model`` key chooses the family: ``"rnampnn"`` = ``RNAMPNN``; a file without the key is an ``rdesign`` checkpoint (the files
``train.py --model rdesign`` has always written).  ``--xgb`` is the tree read-out in XGBoost's JSON schema - without it the read-out's argmax
decides, as in the reference with an unfitted XGBoost head.  ``--data`` holds ``coords/<id>.npy`` (L,7,3) and ``seqs/<id>.fasta`` (optional for
``RNAMPNN``); the CSV has one ``pdb_id,seq`` row per structure in id order.  ``--samples N`` (``RNAMPNN``) also draws N sequences per
structure at ``--temperature`` and writes them with their per-nucleotide NLL and recovery to ``--designs-out``."""
from __future__ import annotations

import argparse
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--ckpt", required=True)
    ap.add_argument("--xgb", default=None)
    ap.add_argument("--data", required=True)
    ap.add_argument("--out", default="submit.csv")
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--samples", type=int, default=0, help="rnampnn: sequences drawn per structure (0 = none)")
    ap.add_argument("--temperature", type=float, default=0.1, help="rnampnn: sampling temperature of --samples")
    ap.add_argument("--seed", type=int, default=0, help="rnampnn: seed of --samples")
    ap.add_argument("--designs-out", default=None, help="rnampnn: CSV of the sampled designs (default: <out>_designs.csv)")
    return ap.parse_args(argv)


def checkpoint_family(path: str) -> str:
    """The ``model`` key of a checkpoint file; a file without one is an ``rdesign`` checkpoint.  ``weights_only=True``."""
    ck = torch.load(path, map_location="cpu", weights_only=True)
    family = ck.get("model", "rdesign") if isinstance(ck, dict) else None
    if family not in ("rnampnn", "rdesign"):
        raise ValueError(f"{path}: unknown model family {family!r}")
    return family


def run(args, log=print):
    family = checkpoint_family(args.ckpt)
    if family == "rnampnn":
        from rnampnn.utils.predict import predict
        from rnampnn.utils.train import load_checkpoint
        extra = dict(samples=args.samples, temperature=args.temperature, seed=args.seed, designs_csv=args.designs_out)
    else:
        from rdesign.utils.predict import predict
        from rdesign.utils.train import load_checkpoint
        if args.samples:
            raise ValueError("--samples belongs to RNAMPNN checkpoints (the rdesign model has no sampler)")
        extra = {}
    model, ck = load_checkpoint(args.ckpt, device=torch.device(args.device))
    if args.xgb:
        model.load_xgb_readout(args.xgb)
    rows = predict(model, args.data, args.out, batch_size=args.batch_size, **extra)
    log(f"{len(rows)} sequences by {ck['name']} v{ck['version']} ({'tree read-out' if args.xgb else 'read-out argmax'}) written to {args.out}")
    return rows


if __name__ == "__main__":
    run(parse())
