"""The epoch loop of the ``rdesign`` model - the role of the reference's ``rdesign/utils/train.py`` (``get_trainer``: Lightning ``Trainer``
+ ``ModelCheckpoint(monitor='val_recovery_rate', mode='max')`` + ``LossMonitor``) without Lightning.  A sibling of
``rnampnn.utils.train.Trainer`` (that class passes ``T_norm`` and overlaps a chunked exchange, neither of which this model has): the same
batch plan (``plan_epoch``), the same per-step seed formula, one process per GPU, ONE flat gradient all-reduce per step, and no host
synchronisation inside an epoch or a validation pass - the loss is accumulated on the device, nucleotide counts come from the loader's
host-side lengths, validation metrics come from ``RNAModel.score_batch`` (``rdesign_score``) as per-RNA device tensors that are reduced
once at the end.  Checkpoints are ``torch.save`` of tensors and plain types, loaded with ``weights_only=True``."""
from __future__ import annotations

import time
from typing import Dict, Optional, Sequence

import torch
import torch.distributed as dist

from rnampnn.utils import shard
from rnampnn.utils.augment import EpochNoise
from rnampnn.utils.data import bucket_batches
from rnampnn.utils.train import plan_epoch

from .data import padded_loader


def validation_metrics(correct: torch.Tensor, valid: torch.Tensor, nll: torch.Tensor) -> Dict[str, float]:
    """``LossMonitor.on_validation_epoch_end`` (rdesign/utils/train.py:25-36) from per-RNA (correct, valid, summed NLL), in float64 and
    summed over the ranks: val_loss = sum(nll) / sum(valid) (token-mean cross-entropy), weighted_val_recovery_rate = sum(correct) /
    sum(valid), val_recovery_rate = mean over the RNAs of correct / valid."""
    micro, macro = shard.reduce_recovery(correct, valid)
    sums = torch.stack([nll.to(torch.float64).sum(), valid.to(torch.float64).sum()])
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        dist.all_reduce(sums, op=dist.ReduceOp.SUM)
    return dict(val_loss=float(sums[0] / sums[1].clamp(min=1)), weighted_val_recovery_rate=micro, val_recovery_rate=macro)


class Trainer:
    """``fit``-style loop around ``RNAModel.loss_and_grad`` + ``allreduce_gradients`` + the optimiser."""

    def __init__(self, model, optimizer, scheduler=None, world: int = 1, rank: int = 0, seed: int = 0):
        self.model, self.opt, self.sched = model, optimizer, scheduler
        self.world, self.rank, self.seed = int(world), int(rank), int(seed)
        self.device = model._device()                     # raises on a CPU module: there is no CPU fallback
        self._loss = torch.zeros((), dtype=torch.float32, device=self.device)
        self.last_validation = None

    def step_seed(self, epoch: int, it: int) -> int:
        """Dropout seed of step ``it`` of ``epoch`` on this rank (the main trainer's formula)."""
        return ((self.seed << 20) + epoch * 100003 + it) * max(self.world, 1) + self.rank

    def plan(self, lengths: Sequence[int], epoch: int, batch_size: int, max_rows: int):
        """This rank's batches (global item indices) of ``epoch``."""
        return plan_epoch(lengths, self.rank, self.world, batch_size, max_rows, self.seed + epoch)[0]

    def step(self, S, X, mask, seed: Optional[int] = None):
        """forward + backward (one native call), gradient exchange, optimiser step; returns the device loss (no sync)."""
        loss = self.model.loss_and_grad(X, S, mask, seed=seed)
        self.model.allreduce_gradients()
        self.opt.step()
        return loss

    def run_epoch(self, items, lengths: Sequence[int], epoch: int, batch_size: int, max_rows: int) -> Dict:
        """One pass over ``items`` ((id, coords, labels) or (coords, labels)); -> dict(train_loss, steps, nt, seconds, nt_per_s) for THIS
        rank's share.  The only host synchronisation is the one at the end of the epoch.  ``items`` may be an ``AugmentedItems``
        (``lengths`` = its virtual lengths): its noisy samples get their noise on the device ahead of each step, on the six atoms the
        loader keeps; ``validate`` never augments."""
        self.model.train()
        mine = self.plan(lengths, epoch, batch_size, max_rows)
        loader = padded_loader(items, mine, device=self.device)
        self.model.reserve_training((len(b), max(int(lengths[i]) for i in b)) for b in mine)
        noise = EpochNoise.of(items, mine, self.device)     # AugmentedItems with noisy samples: this epoch's (sigma, key, offset) rows, uploaded once
        self._loss.zero_()
        torch.cuda.synchronize(self.device)
        t0 = time.perf_counter()
        nt = 0
        for it, (S, X, mask, lens, _) in enumerate(loader):
            if noise is not None:
                X = noise.apply(it, X, mask)
            self._loss += self.step(S, X, mask, seed=self.step_seed(epoch, it))
            nt += sum(lens)
        if self.sched is not None:
            self.sched.step()
        torch.cuda.synchronize(self.device)
        dt = time.perf_counter() - t0
        steps = len(mine)
        return dict(train_loss=float(self._loss) / max(steps, 1), steps=steps, nt=nt, seconds=dt, nt_per_s=nt / dt)

    @torch.no_grad()
    def validate(self, items, lengths: Sequence[int], batch_size: int, max_rows: int, use_trees: bool = False) -> Dict[str, float]:
        """-> dict(val_loss, weighted_val_recovery_rate, val_recovery_rate) over all ranks (``validation_metrics``); every rank scores a
        strided share of the length-bucketed batches.  ``use_trees``: score the tree read-out instead (val_loss is then NaN)."""
        self.model.eval()
        batches = bucket_batches(lengths, batch_size, max_rows, seed=0)[self.rank::self.world]
        cs, vs, ls = [], [], []
        for S, X, mask, lens, _ in padded_loader(items, batches, device=self.device):
            c, v, l = self.model.score_batch(X, S, mask, lengths=lens, use_trees=use_trees)
            cs.append(c); vs.append(v)
            if l is not None:
                ls.append(l)
        cat = lambda parts, dt: torch.cat(parts) if parts else torch.zeros(0, dtype=dt, device=self.device)
        c, v, l = cat(cs, torch.int32), cat(vs, torch.int32), cat(ls, torch.float32)
        self.last_validation = dict(correct=c, valid=v, nll=l)          # this rank's per-RNA tensors, in batch order
        out = validation_metrics(c, v, l)
        if use_trees:
            out["val_loss"] = float("nan")
        return out


# ---------------------------------------------------------------------------------------------------------------- checkpoints
def save_checkpoint(path: str, model, name: Optional[str] = None, version: Optional[int] = None, **extra) -> None:
    """``Final.pt``: state_dict (CPU tensors) + constructor kwargs + name / version (+ plain-typed ``extra``, e.g. the epoch and its
    ``val_recovery_rate``).  Tensors and plain types only, so ``torch.load(weights_only=True)`` reads it back."""
    torch.save(dict(state_dict={k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, init_kwargs=dict(model.init_kwargs),
                    name=str(model.name if name is None else name), version=int(model.version if version is None else version), **extra), path)


def load_checkpoint(path: str, device=None):
    """-> (RNAModel rebuilt from a ``save_checkpoint`` file, the file's dict).  ``weights_only=True``: pickled objects are never loaded."""
    from ..model.rdesign import RNAModel
    ck = torch.load(path, map_location="cpu", weights_only=True)
    model = RNAModel(**ck["init_kwargs"])
    model.load_state_dict(ck["state_dict"])
    model.name, model.version = ck["name"], ck["version"]
    if device is not None:
        model = model.to(device)
    return model, ck
