#!/usr/bin/env python3
"""Design sequences for a directory of structures with a trained ``rdesign`` model - the role of the reference's ``main.py:17-31``:

    python rna-mpnn_amd/predict.py --ckpt runs/rdesign/Final.pt [--xgb runs/rdesign/XGB.json] --data /path/to/data --out submit.csv

``--ckpt`` is what ``train.py --model rdesign --out DIR`` wrote (weights + constructor arguments, loaded with ``weights_only=True``; pickles
are never loaded), ``--xgb`` the tree read-out in XGBoost's JSON schema - without it the read-out's argmax decides, as in the reference
with an unfitted XGBoost head.  ``--data`` holds ``coords/<id>.npy`` (L,7,3) and ``seqs/<id>.fasta``; the CSV has one ``pdb_id,seq`` row
per structure in id order."""
from __future__ import annotations

import argparse
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from rdesign.utils.predict import predict  # noqa: E402
from rdesign.utils.train import load_checkpoint  # noqa: E402


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--ckpt", required=True)
    ap.add_argument("--xgb", default=None)
    ap.add_argument("--data", required=True)
    ap.add_argument("--out", default="submit.csv")
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--device", default="cuda:0")
    return ap.parse_args(argv)


def run(args, log=print):
    model, ck = load_checkpoint(args.ckpt, device=torch.device(args.device))
    if args.xgb:
        model.load_xgb_readout(args.xgb)
    rows = predict(model, args.data, args.out, batch_size=args.batch_size)
    log(f"{len(rows)} sequences by {ck['name']} v{ck['version']} ({'tree read-out' if args.xgb else 'read-out argmax'}) written to {args.out}")
    return rows


if __name__ == "__main__":
    run(parse())
