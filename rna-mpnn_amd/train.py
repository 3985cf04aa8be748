#!/usr/bin/env python3
"""Drop-in training driver for the MI355X RNA-MPNN path (the role of the reference's ``train.py:1-59`` +
``rnampnn/utils/train.py:91-118`` without Lightning): Adam(lr=2e-3, wd=2e-4) + StepLR(15, 0.8)
(``rnampnn.py:156-159``), loss = cross_entropy(softmax(logits)) (``rnampnn.py:151-154``), macro / micro
recovery on a validation split (``utils/train.py:15-26``).  Gradients come from the HIP backward; data-parallel
runs are one process per GPU with ONE flat RCCL all-reduce per step (``RNAMPNN.allreduce_gradients``):

    python rna-mpnn_amd/train.py --data /path/to/data --epochs 2                    # coords/*.npy + seqs/*.fasta
    python rna-mpnn_amd/train.py --synthetic 512 --epochs 3                         # seeded synthetic RNAs
    python rna-mpnn_amd/train.py --data /path/to/data --epochs 60 --fit-xgb --out runs/rnampnn           # Final.pt (best epoch), last.pt, XGB.json
    python rna-mpnn_amd/train.py --data /path/to/data --epochs 60 --out runs/rnampnn --resume runs/rnampnn/last.pt
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 rna-mpnn_amd/train.py --synthetic 4096
    python rna-mpnn_amd/train.py --model rdesign --data /path/to/data --epochs 230 --fit-xgb --out runs/rdesign   # the sibling model

Batches are length-bucketed (``rnampnn.utils.train.plan_epoch``): the reference's collate pads every RNA of a batch
to the longest one, so mixing a 2,436-nt ribosomal RNA with 20-nt hairpins would spend > 99 % of the rows on padding.
The loop itself is ``rnampnn.utils.train.Trainer``: inputs through ``PaddedLoader`` (pinned memory, copies on a side stream),
loss accumulated on the device, no host synchronisation inside an epoch or a validation pass (``Trainer.validate_metrics``: per-RNA
scores from ``rnampnn_score``).  ``--out DIR`` keeps ``Final.pt`` of the epoch with the best ``val_recovery_rate`` (the reference's
``ModelCheckpoint``, ``rnampnn/utils/train.py:98-104``) and ``last.pt`` with optimiser and scheduler state, which ``--resume`` continues from.

``--model rdesign`` trains the reference's sibling model instead (the reference's own ``train.py:62-80``: ``rdesign.model.rdesign.RNAModel``,
Adam(lr) + StepLR(40, 0.8), checkpoint of the epoch with the best ``val_recovery_rate``, XGBoost head fitted at the end) through
``rdesign.utils.train.Trainer``; ``--out DIR`` receives ``Final.pt`` (and ``XGB.json`` with ``--fit-xgb``), which ``predict.py`` reads.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from rnampnn.model.rnampnn import RNAMPNN  # noqa: E402
from rnampnn.utils import synth  # noqa: E402
from rnampnn.utils.data import PaddedLoader, bucket_batches, load_rna_dir  # noqa: E402
from rnampnn.utils.train import Trainer, load_checkpoint, save_checkpoint  # noqa: E402


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="rnampnn", choices=["rnampnn", "rdesign"],
                    help="rnampnn = RNAMPNN (the default); rdesign = the sibling RNAModel (6 backbone atoms, k = 25, 9 layers, dropout 0.1)")
    ap.add_argument("--data", default=None)
    ap.add_argument("--synthetic", type=int, default=0)
    ap.add_argument("--lengths-file", default=None,
                    help="synthetic RNAs of exactly these lengths (.npy int array; tests/data/c3_train_lengths.npy = the 2,083 ids of the "
                         "reference's data/train_data.csv)")
    ap.add_argument("--epochs", type=int, default=1)
    ap.add_argument("--batch-size", type=int, default=512, help="upper bound on RNAs per step per rank")
    ap.add_argument("--max-nt", type=int, default=32768, help="upper bound on padded rows (B*T) of one step per rank")
    ap.add_argument("--max-len", type=int, default=4500, help="longest RNA kept (= padding_len; the reference trained with 100, train.py:57)")
    ap.add_argument("--neighbours", type=int, default=None, help="default: 30 (rnampnn), 25 (rdesign)")
    ap.add_argument("--layers", type=int, default=None, help="default: 10 (rnampnn), 9 (rdesign)")
    ap.add_argument("--dropout", type=float, default=None, help="default: the reference's 0.4 (rnampnn.py:47); rdesign: 0.1")
    ap.add_argument("--nan-policy", default="skip", choices=["skip", "fill"])
    ap.add_argument("--train-precision", default="bf16", choices=["bf16", "f32"],
                    help="bf16 = the reference's bf16-mixed trainer setting (utils/train.py:109); f32 = exact")
    ap.add_argument("--torch-adam", action="store_true", help="torch.optim.Adam instead of the fused flat-buffer Adam")
    ap.add_argument("--global-t-norm", action="store_true",
                    help="normalise with the MAX padded length over the ranks (an N-rank step == the 1-rank step on the union batch); "
                         "default: each rank its own batch length, as the reference's DDP ranks do")
    ap.add_argument("--no-validation", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--fit-xgb", action="store_true",
                    help="after the last epoch fit the gradient-boosted-tree read-out on the training embeddings, on the device "
                         "(the reference's XGBTrainer.on_fit_end, utils/train.py:50-75) and print train / validation score")
    ap.add_argument("--xgb-out", default=None, help="with --fit-xgb: write the fitted model as XGBoost-schema JSON")
    ap.add_argument("--out", default=None,
                    help="directory for Final.pt (weights of the epoch with the best val_recovery_rate + constructor arguments) and, with "
                         "--fit-xgb, XGB.json; --model rnampnn also writes last.pt (weights, optimiser and scheduler state) after every epoch")
    ap.add_argument("--resume", default=None, metavar="FILE",
                    help="--model rnampnn: continue from a last.pt - weights, optimiser, scheduler and epoch counter (--epochs is the total)")
    ap.add_argument("--noise-augmentation", type=int, default=0, metavar="N",
                    help="N noisy copies of training RNAs drawn with replacement, coordinates + N(0, --noise-std^2) added on the device "
                         "(the reference's RNADataset.noise_augmentation, utils/data.py:278-295); training split only")
    ap.add_argument("--slice-augmentation", type=int, default=0, metavar="N",
                    help="N windows of exactly --slice-len residues cut from training RNAs (noisy copies included) longer than that "
                         "(RNADataset.slice_augmentation, utils/data.py:297-324); training split only")
    ap.add_argument("--slice-len", type=int, default=1000, help="window length of --slice-augmentation (the reference's MIN_LEN)")
    ap.add_argument("--noise-std", type=float, default=1e-2, help="standard deviation of --noise-augmentation's noise")
    ap.add_argument("--augment-eps", type=float, default=0.0,
                    help="--model rdesign: X + eps * N(0, 1) on every training step (the reference's RNAFeatures(augment_eps))")
    return ap.parse_args(argv)


def rdesign_precisions(train_precision: str) -> dict:
    """--train-precision -> RNAModel's two precision arguments: bf16 (the CLI default) = bf16 inference + the bf16-mixed step; f32 = the
    reference's arithmetic, exact-f32 inference and step."""
    return dict(precision="bf16", train_precision="bf16") if train_precision == "bf16" else dict(precision="f32", train_precision="f32")


def _init_dist():
    rank, world, local = (int(os.environ.get(k, d)) for k, d in (("RANK", "0"), ("WORLD_SIZE", "1"), ("LOCAL_RANK", "0")))
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    torch.cuda.set_device(local)
    return rank, world, torch.device("cuda", local)


def _synthetic_items(args):
    if args.lengths_file:
        lens = [int(n) for n in np.load(args.lengths_file, allow_pickle=False) if 0 < int(n) <= args.max_len]
    else:
        lens = synth.synth_lengths(args.synthetic or 256, 30, min(140, args.max_len), seed=1)
    return [(synth.synth_rna(int(n), i, seed=1), synth.synth_labels(int(n), i, seed=1)) for i, n in enumerate(lens)]


def _augment(train, train_lens, args):
    """--noise-augmentation / --slice-augmentation -> (training items, their lengths).  The TRAINING split only: the reference augments the
    whole set before it splits (utils/data.py:402-438), which puts noisy copies of training RNAs into validation.  With both flags at 0
    the list comes back as it is."""
    if args.noise_augmentation or args.slice_augmentation:
        from rnampnn.utils.augment import AugmentedItems
        train = AugmentedItems(train, noise=args.noise_augmentation, slices=args.slice_augmentation, min_len=args.slice_len,
                               noise_std=args.noise_std, seed=args.seed)
        return train, [int(n) for n in train.lengths]
    return train, train_lens


def _split(items, args):
    n_val = 0 if args.no_validation else max(1, len(items) // 20)
    order0 = np.random.RandomState(args.seed).permutation(len(items))          # id-order-independent split
    return [items[i] for i in order0[n_val:]], [items[i] for i in order0[:n_val]]


def run(args, log=print):
    """-> dict(epochs=[dict(train_loss, val_loss, weighted_val_recovery_rate, val_recovery_rate, val_micro, val_macro, nt_per_s, steps,
    seconds)], n_train, n_val, best_epoch, model[, xgb]).  ``--out DIR``: ``Final.pt`` whenever ``val_recovery_rate`` improves (no
    validation split: every epoch, so the last one stays) and ``last.pt`` with optimiser / scheduler state after every epoch, written
    by rank 0 ahead of a barrier; ``--resume FILE`` continues from such a ``last.pt``."""
    if args.model == "rdesign":
        if args.resume:
            raise ValueError("--resume belongs to --model rnampnn (the rdesign trainer writes no last.pt)")
        return run_rdesign(args, log)
    if args.augment_eps:
        raise ValueError("--augment-eps belongs to --model rdesign (the reference's RNAMPNN has no such argument)")
    rank, world, dev = _init_dist()
    if args.data:
        items = [(c, y) for _, c, y in load_rna_dir(args.data, max_len=args.max_len, nan_policy=args.nan_policy)]
    else:
        items = _synthetic_items(args)
    train, val = _split(items, args)
    hp = dict(num_res_neighbours=args.neighbours or 30, num_res_mpnn_layers=args.layers or 10, padding_len=max(args.max_len, 1))
    if args.dropout is not None:
        hp["dropout"] = args.dropout
    resume = None
    if args.resume:                                 # every rank reads the same file: identical weights without a broadcast
        model, resume = load_checkpoint(args.resume, device=dev)
    else:
        model = RNAMPNN(**hp).to(dev)
    model.train_precision = args.train_precision
    if world > 1 and resume is None:                # identical initial weights on every rank
        for p in model.parameters():
            dist.broadcast(p.data, 0)
        model._weights_touched()
    (opt,), (sched,) = model.configure_optimizers(fused=not args.torch_adam)
    if resume is not None:
        if "optimizer" not in resume or "epoch" not in resume:
            raise ValueError(f"{args.resume} carries no optimiser state / epoch counter: --resume takes the last.pt that --out writes")
        opt.load_state_dict(resume["optimizer"])
        if "scheduler" in resume:
            sched.load_state_dict(resume["scheduler"])
    trainer = Trainer(model, opt, sched, world=world, rank=rank, global_t_norm=args.global_t_norm, seed=args.seed)
    train_lens = [c.shape[0] for c, _ in train]
    val_lens = [c.shape[0] for c, _ in val]
    epoch_items, epoch_lens = _augment(train, train_lens, args)         # the tree read-out below is fitted on the plain training RNAs
    out = dict(epochs=[], n_train=len(epoch_items), n_val=len(val), best_epoch=None)
    final = os.path.join(args.out, "Final.pt") if args.out else None
    last = os.path.join(args.out, "last.pt") if args.out else None
    if args.out and rank == 0:
        os.makedirs(args.out, exist_ok=True)
    best, nan = float("-inf"), float("nan")
    first = 0
    if resume is not None:
        first = int(resume["epoch"]) + 1
        if resume.get("best_epoch", -1) >= 0:
            best, out["best_epoch"] = float(resume["best_val_recovery_rate"]), int(resume["best_epoch"])
    for epoch in range(first, args.epochs):
        rec = trainer.run_epoch(epoch_items, epoch_lens, epoch, args.batch_size, args.max_nt)
        if world > 1:       # whole-job rate: all nucleotides / slowest rank
            t = torch.tensor([rec["seconds"], float(rec["nt"])], dtype=torch.float64, device=dev)
            tmax = t.clone(); dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
            rec["nt_per_s"] = float(t[1] / tmax[0])
        rec.update(trainer.validate_metrics(val, val_lens, args.batch_size, args.max_nt) if val
                   else dict(val_loss=nan, weighted_val_recovery_rate=nan, val_recovery_rate=nan))
        micro, macro = rec["weighted_val_recovery_rate"], rec["val_recovery_rate"]      # (what Trainer.validate returns, from the same counts)
        rec.update(val_micro=micro, val_macro=macro)
        out["epochs"].append(rec)
        if not val or out["best_epoch"] is None or macro > best:        # ModelCheckpoint(monitor='val_recovery_rate', mode='max'); no split: the last epoch
            best, out["best_epoch"] = macro, epoch
            if final and rank == 0:
                save_checkpoint(final, model, epoch=epoch, val_recovery_rate=float(macro), val_loss=float(rec["val_loss"]))
        if last and rank == 0:
            save_checkpoint(last, model, opt, sched, epoch=epoch, val_recovery_rate=float(macro), best_epoch=int(out["best_epoch"]),
                            best_val_recovery_rate=float(best))
        if args.out and world > 1:
            dist.barrier()
        if rank == 0:
            log(f"epoch {epoch}: train_loss {rec['train_loss']:.4f}  val_recovery micro {micro:.4f} macro {macro:.4f}  "
                f"{rec['nt_per_s']:.0f} nt/s end to end ({rec['steps']} steps, {rec['seconds']:.2f} s, {world} rank(s))")
    if final and out["epochs"]:
        if args.fit_xgb and out["best_epoch"] != args.epochs - 1:      # XGBTrainer.on_fit_end reloads the Final checkpoint before the fit
            model.load_state_dict(load_checkpoint(final)[1]["state_dict"])
        if rank == 0:
            log(f"checkpoint of epoch {out['best_epoch']} written to {final}")
    if args.fit_xgb and rank == 0:
        out["xgb"] = fit_xgb(model, train, train_lens, val, val_lens, args, dev, log)
        if args.out:
            model.xgb_readout.save_json(os.path.join(args.out, "XGB.json"))
            log(f"tree read-out written to {os.path.join(args.out, 'XGB.json')}")
    out["model"] = model
    return out


def run_rdesign(args, log=print):
    """``--model rdesign`` -> dict(epochs=[dict(train_loss, val_loss, weighted_val_recovery_rate, val_recovery_rate, nt_per_s, steps,
    seconds)], n_train, n_val, best_epoch, model[, xgb]).  The model that is returned (and that the tree read-out is fitted on) carries
    the weights of the best epoch, as the reference's ``XGBTrainer`` reloads its ``Final`` checkpoint."""
    from rdesign.model.rdesign import RNAModel
    from rdesign.utils import data as rdata
    from rdesign.utils.train import Trainer as RDesignTrainer, load_checkpoint, save_checkpoint
    rank, world, dev = _init_dist()
    if args.data:
        items = [(c, y) for _, c, y in rdata.load_rna_dir(args.data, max_len=args.max_len)]        # missing atoms -> 0, as the reference's collate
    else:
        items = _synthetic_items(args)                                                             # 7-atom records: the loader keeps the first six
    train, val = _split(items, args)
    kw = dict(k_neighbors=args.neighbours or 25, num_mpnn_layers=args.layers or 9, **rdesign_precisions(args.train_precision))
    if args.augment_eps:
        kw["augment_eps"] = args.augment_eps
    if args.dropout is not None:
        kw["dropout"] = args.dropout
    model = RNAModel(**kw).to(dev)
    if world > 1:                                   # identical initial weights on every rank
        for p in model.parameters():
            dist.broadcast(p.data, 0)
        model._weights_touched()
    (opt,), (sched,) = model.configure_optimizers(fused=not args.torch_adam)
    trainer = RDesignTrainer(model, opt, sched, world=world, rank=rank, seed=args.seed)
    train_lens = [c.shape[0] for c, _ in train]
    val_lens = [c.shape[0] for c, _ in val]
    epoch_items, epoch_lens = _augment(train, train_lens, args)         # the tree read-out below is fitted on the plain training RNAs
    out = dict(epochs=[], n_train=len(epoch_items), n_val=len(val), best_epoch=None)
    ckpt = os.path.join(args.out, "Final.pt") if args.out else None
    if ckpt and rank == 0:
        os.makedirs(args.out, exist_ok=True)
    best, nan = float("-inf"), float("nan")
    for epoch in range(args.epochs):
        rec = trainer.run_epoch(epoch_items, epoch_lens, epoch, args.batch_size, args.max_nt)
        if world > 1:       # whole-job rate: all nucleotides / slowest rank
            t = torch.tensor([rec["seconds"], float(rec["nt"])], dtype=torch.float64, device=dev)
            tmax = t.clone(); dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
            rec["nt_per_s"] = float(t[1] / tmax[0])
        rec.update(trainer.validate(val, val_lens, args.batch_size, args.max_nt) if val
                   else dict(val_loss=nan, weighted_val_recovery_rate=nan, val_recovery_rate=nan))
        out["epochs"].append(rec)
        score = rec["val_recovery_rate"]
        if not val or out["best_epoch"] is None or score > best:        # ModelCheckpoint(monitor='val_recovery_rate', mode='max'); no split: the last epoch
            best, out["best_epoch"] = score, epoch
            if ckpt and rank == 0:
                save_checkpoint(ckpt, model, epoch=epoch, val_recovery_rate=float(score))
        if rank == 0:
            log(f"epoch {epoch}: train_loss {rec['train_loss']:.4f}  val_loss {rec['val_loss']:.4f}  val_recovery_rate {score:.4f} "
                f"(weighted {rec['weighted_val_recovery_rate']:.4f})  {rec['nt_per_s']:.0f} nt/s end to end "
                f"({rec['steps']} steps, {rec['seconds']:.2f} s, {world} rank(s))")
    if ckpt:
        if world > 1:
            dist.barrier()
        if out["best_epoch"] != args.epochs - 1:
            model.load_state_dict(load_checkpoint(ckpt)[1]["state_dict"])
        if rank == 0:
            log(f"checkpoint of epoch {out['best_epoch']} written to {ckpt}")
    if args.fit_xgb and rank == 0:
        out["xgb"] = fit_xgb(model, train, train_lens, val, val_lens, args, dev, log, atoms=6)
        if args.out:
            model.xgb_readout.save_json(os.path.join(args.out, "XGB.json"))
            log(f"tree read-out written to {os.path.join(args.out, 'XGB.json')}")
    out["model"] = model
    return out


def fit_xgb(model, train, train_lens, val, val_lens, args, dev, log=print, atoms=7):
    """``XGBTrainer.on_fit_end``: embeddings of every valid training nucleotide -> tree read-out fitted on the device -> train and
    validation score; the embeddings never leave the device."""
    model.eval()
    loader = lambda items, lens: PaddedLoader(items, bucket_batches(lens, args.batch_size, args.max_nt, seed=0), device=dev, atoms=atoms)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    train_score = model.fit_xgb_readout(loader(train, train_lens), seed=args.seed)
    torch.cuda.synchronize(dev)
    rec = dict(train_score=train_score, val_score=float("nan"), seconds=time.perf_counter() - t0, trees=len(model.xgb_readout.arrays["tree_class"]))
    if val:
        X, y = model.embed_valid(loader(val, val_lens))
        rec["val_score"] = model.xgb_readout.score(X, y)
    log(f"tree read-out: {rec['trees']} trees fitted in {rec['seconds']:.2f} s (embedding included)  "
        f"training score {rec['train_score']:.4f}  validation score {rec['val_score']:.4f}")
    if args.xgb_out:
        model.xgb_readout.save_json(args.xgb_out)
        log(f"tree read-out written to {args.xgb_out}")
    return rec


def main():
    run(parse())
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
