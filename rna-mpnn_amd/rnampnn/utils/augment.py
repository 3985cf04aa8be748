"""The reference's training-set augmentations on the MI355X path: ``RNADataset.noise_augmentation`` / ``slice_augmentation``
(``rnampnn/utils/data.py:278-324``, applied by ``RNADataModule``, ``data.py:402-438``) and ``RNAFeatures(augment_eps)`` of the
``rdesign`` sibling (``rdesign/model/feature.py:157-158``).

Nothing is stored: the noise of a coordinate is a pure function of (sample key, residue index in the SOURCE RNA, atom, axis) -
``rnampnn_augment_coords`` (``csrc/augment.hip``) adds it to a padded batch on the device - so a "noisy copy" is a row of a small table
(source, sigma, key, offset) and a slice is a numpy view.  The copies are the same in every epoch (as the reference's stored ones are), on
every rank and in whatever batch they land, and a slice of a noisy copy carries exactly that copy's noise.

* ``noise_reference``  - numpy restatement of the kernel (``synth.normal01`` in f64, one f32 add): the checker of the tests.
* ``augment_coords``   - the native call on the current stream.
* ``AugmentedItems``   - read-only ``Sequence`` of virtual samples: the originals, then the noisy copies, then the slices.
* ``EpochNoise``       - the per-step (sigma, key, offset) rows of one epoch plan, uploaded once; what the two trainers apply.
"""
from __future__ import annotations

import ctypes as C
from collections.abc import Sequence as _Sequence
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import synth

_M64 = (1 << 64) - 1


# --------------------------------------------------------------------------------------------------------------- the generator, restated
def row_stream(seed: int, b: int) -> int:
    """Stream of batch row ``b`` when no key is given (``include/rnampnn_hip.h``): mix64(mix64(seed) + (b + 1) * 0x9E3779B97F4A7C15)."""
    s = int(synth._mix64(np.array([int(seed) & _M64], dtype=np.uint64))[0])
    return int(synth._mix64(np.array([(s + (int(b) + 1) * synth._GOLDEN) & _M64], dtype=np.uint64))[0])


def noise_reference(coords, length: int, sigma: float, key: int, offset: int = 0) -> np.ndarray:
    """What ``rnampnn_augment_coords`` computes for ONE batch row: coords (T, atoms, 3) f32 with ``length`` valid residues ->
    a copy whose value (t, a, x), t < length, is ``coords + f32(sigma * normal01(key, ((offset + t) * atoms + a) * 3 + x))`` - the normal in
    f64 (``synth.normal01``), the product rounded to f32 once, one f32 add.  ``sigma == 0`` and the residues t >= length: the input's bits."""
    c = np.array(coords, dtype=np.float32, copy=True)
    n, sg = int(length), np.float32(sigma)
    if sg == 0 or n <= 0:
        return c
    per = int(c.shape[1]) * 3
    idx = (np.arange(n * per, dtype=np.int64) + int(offset) * per).astype(np.uint64)
    z = synth.normal01(int(key) & _M64, idx).reshape(n, c.shape[1], 3)
    c[:n] = c[:n] + (np.float64(sg) * z).astype(np.float32)
    return c


# --------------------------------------------------------------------------------------------------------------- the native call
def augment_coords(coords: torch.Tensor, mask: torch.Tensor, sigma: torch.Tensor, key: Optional[torch.Tensor] = None,
                   offset: Optional[torch.Tensor] = None, seed: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``rnampnn_augment_coords`` on the current stream of ``coords``' device: coords (B, T, atoms, 3) f32 with atoms 6 or 7, mask (B, T)
    f32 prefix masks, sigma (B,) f32, key (B,) 64-bit integers or None (then row b draws from ``row_stream(seed, b)``), offset (B,) int32
    or None (= 0); all on the device already - nothing is copied or synchronised here.  ``out``: None = a new tensor, or ``coords``
    itself (in place).  Rows with sigma 0 and padded residues come back bit for bit."""
    from .. import _native
    dev = coords.device
    if dev.type != "cuda":
        raise RuntimeError("augment_coords runs on an MI355X: pass device tensors (there is no CPU fallback; noise_reference is the checker)")
    if coords.dim() != 4 or coords.shape[3] != 3 or coords.dtype != torch.float32 or not coords.is_contiguous():
        raise ValueError(f"coords must be a contiguous f32 (B, T, atoms, 3) tensor, got {tuple(coords.shape)} {coords.dtype}")
    B, T, atoms = int(coords.shape[0]), int(coords.shape[1]), int(coords.shape[2])

    def arg(t, name, shape, dtypes):
        if t is None:
            return None
        if t.device != dev or tuple(t.shape) != shape or t.dtype not in dtypes or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {dtypes[0]} tensor of shape {shape} on {dev}, got {tuple(t.shape)} {t.dtype} on {t.device}")
        return C.c_void_p(t.data_ptr())

    pm = arg(mask, "mask", (B, T), (torch.float32,))
    ps = arg(sigma, "sigma", (B,), (torch.float32,))
    pk = arg(key, "key", (B,), (torch.int64, torch.uint64))
    po = arg(offset, "offset", (B,), (torch.int32,))
    if pm is None or ps is None:
        raise ValueError("mask and sigma are required")
    if out is None:
        out = torch.empty_like(coords)
    elif out is not coords and (out.shape != coords.shape or out.dtype != torch.float32 or out.device != dev or not out.is_contiguous()):
        raise ValueError("out must be coords itself or a contiguous f32 tensor of its shape on its device")
    with torch.cuda.device(dev):
        _native.check(_native.lib().rnampnn_augment_coords(C.c_void_p(coords.data_ptr()), pm, B, T, atoms, ps, pk, po,
                                                           C.c_uint64(int(seed) & _M64), C.c_void_p(out.data_ptr()),
                                                           C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return out


# --------------------------------------------------------------------------------------------------------------- virtual samples
def _draw(name: str, seed: int, count: int, n: int) -> np.ndarray:
    """``count`` integers uniform in [0, n) from the named counter stream (24-bit uniforms: n < 2^24)."""
    u = synth.uniform01(synth._fnv1a64(f"augment/{name}/{int(seed)}"), np.arange(count, dtype=np.uint64))
    return np.minimum(np.floor(u * n).astype(np.int64), n - 1)


class AugmentedItems(_Sequence):
    """Read-only sequence of VIRTUAL training samples over ``items`` ((id, coords, labels) tuples or (coords, labels) pairs): the
    originals, then ``noise`` noisy copies, then ``slices`` slices.  ``[i]`` is an item of the source's form whose coordinates and labels
    are numpy views of the source (``src[start:start + length]``; a whole RNA is the source item itself); the noise is not in the arrays,
    it is the sample's row of ``sigma`` (f32) / ``key`` (u64) / ``offset`` (i32), which ``rnampnn_augment_coords`` applies on the device.
    ``lengths`` and ``source`` (index into ``items``) complete the table.

    Noisy copy j: source uniform with replacement among the ORIGINALS, sigma = ``noise_std``, key = a hash of (seed, j), offset 0.  (The
    reference's loop appends as it goes, so it can draw an earlier noisy copy and noise it twice; that accident is not restated.)
    Slice j: source uniform among all originals and noisy copies LONGER than ``min_len``, start uniform in [0, L - min_len], length exactly
    ``min_len``; it inherits the source's sigma and key, with offset = start.  No such source: ``ValueError``, as the reference raises.
    Every draw comes from ``synth.uniform01`` on a stream named by ``seed``: no ``numpy.random`` / ``random`` state, every rank builds the
    same set.  With ``noise == slices == 0`` the sequence is the identity over ``items``."""

    def __init__(self, items: Sequence, noise: int = 0, slices: int = 0, min_len: int = 1000, noise_std: float = 1e-2, seed: int = 0):
        noise, slices, min_len = int(noise), int(slices), int(min_len)
        if noise < 0 or slices < 0 or min_len < 1 or not float(noise_std) >= 0.0:
            raise ValueError("noise and slices must be >= 0, min_len >= 1, noise_std >= 0")
        self.items = items
        self.n_original, self.noise, self.slices = len(items), noise, slices
        self.min_len, self.noise_std, self.seed = min_len, float(noise_std), int(seed)
        n0 = self.n_original
        if n0 >= 1 << 24 or n0 + noise >= 1 << 24:
            raise ValueError("more than 2^24 samples: the 24-bit draws would skip some")
        len0 = np.array([int(self._coords(it).shape[0]) for it in items], dtype=np.int64)
        n = n0 + noise + slices
        self.source = np.zeros(n, dtype=np.int64)
        self.lengths = np.zeros(n, dtype=np.int64)
        self.sigma = np.zeros(n, dtype=np.float32)
        self.key = np.zeros(n, dtype=np.uint64)
        self.offset = np.zeros(n, dtype=np.int32)
        self.source[:n0], self.lengths[:n0] = np.arange(n0), len0
        if noise:
            if n0 == 0:
                raise ValueError("no items to draw noisy copies from")
            src = _draw("noise_source", seed, noise, n0)
            self.source[n0:n0 + noise], self.lengths[n0:n0 + noise] = src, len0[src]
            self.sigma[n0:n0 + noise] = np.float32(noise_std)
            self.key[n0:n0 + noise] = [synth._fnv1a64(f"augment/noise_key/{int(seed)}/{j}") for j in range(noise)]
        if slices:
            pool = np.nonzero(self.lengths[:n0 + noise] > min_len)[0]           # virtual indices: originals and noisy copies
            if len(pool) == 0:
                raise ValueError("No sequences longer than min_len available for slicing.")
            pick = pool[_draw("slice_source", seed, slices, len(pool))]
            u = synth.uniform01(synth._fnv1a64(f"augment/slice_start/{int(seed)}"), np.arange(slices, dtype=np.uint64))
            room = self.lengths[pick] - min_len                                    # start in [0, room], inclusive
            start = np.minimum(np.floor(u * (room + 1)).astype(np.int64), room)
            s0 = n0 + noise
            self.source[s0:], self.lengths[s0:] = self.source[pick], min_len
            self.sigma[s0:], self.key[s0:], self.offset[s0:] = self.sigma[pick], self.key[pick], start.astype(np.int32)
        for a in (self.source, self.lengths, self.sigma, self.key, self.offset):
            a.setflags(write=False)

    @staticmethod
    def _coords(it):
        return it[1] if len(it) == 3 else it[0]

    @property
    def augments(self) -> bool:
        """True when some sample carries noise (the trainers then run the device kernel ahead of every step)."""
        return bool((self.sigma > 0).any())

    def __len__(self) -> int:
        return len(self.lengths)

    def __getitem__(self, i):
        i = int(i)
        if i < 0:
            i += len(self)
        if not 0 <= i < len(self):
            raise IndexError(i)
        it = self.items[int(self.source[i])]
        s, n = int(self.offset[i]), int(self.lengths[i])
        if s == 0 and n == int(self._coords(it).shape[0]):
            return it                                   # a whole RNA (an original or a noisy copy): the source item itself
        if len(it) == 3:
            return (it[0], it[1][s:s + n], it[2][s:s + n])
        return (it[0][s:s + n], it[1][s:s + n])


# --------------------------------------------------------------------------------------------------------------- what a trainer applies
class EpochNoise:
    """The (sigma, key, offset) rows of every step of one epoch plan (``batches``: lists of virtual indices, in step order), concatenated
    and uploaded ONCE - before the epoch's clock starts - so a step costs one kernel on a view of them: no per-step host-to-device copy,
    no synchronisation.  ``EpochNoise.of`` returns None for plain items and for sets without noise: the trainers then take today's path."""

    def __init__(self, items: AugmentedItems, batches: Sequence[Sequence[int]], device):
        flat = np.array([i for b in batches for i in b], dtype=np.int64)
        self.bounds = np.concatenate([[0], np.cumsum([len(b) for b in batches])]).astype(np.int64)
        self.noisy: List[bool] = [bool((items.sigma[list(b)] > 0).any()) for b in batches]
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        self.sigma = up(items.sigma[flat])
        self.key = up(items.key[flat].view(np.int64))
        self.offset = up(items.offset[flat])

    @staticmethod
    def of(items, batches, device) -> Optional["EpochNoise"]:
        return EpochNoise(items, batches, device) if isinstance(items, AugmentedItems) and items.augments else None

    def apply(self, step: int, coords: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
        """Noise the device batch of step ``step`` in place (a step whose rows all have sigma 0 launches nothing: the kernel would copy)."""
        if not self.noisy[step]:
            return coords
        lo, hi = int(self.bounds[step]), int(self.bounds[step + 1])
        return augment_coords(coords, mask, self.sigma[lo:hi], self.key[lo:hi], self.offset[lo:hi], out=coords)
