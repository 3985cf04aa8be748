"""GPU tests of the training-set augmentations: ``rnampnn_augment_coords`` against its numpy restatement (``noise_reference``), its
bit-for-bit contracts (plain rows, padding, in place, repeatability, independence of the batch a sample lands in), and the two trainers
and the ``rdesign`` model's ``augment_eps`` on top of it.  Smallest shapes that can still go wrong: B = 3, T = 9, lengths [9, 1, 4], with
7 atoms (21 values per residue, an odd count) and with 6."""
import numpy as np
import pytest
import torch

from rnampnn.utils import synth
from rnampnn.utils.augment import AugmentedItems, EpochNoise, augment_coords, noise_reference, row_stream

pytestmark = pytest.mark.gpu

LENS = [9, 1, 4]
SIGMA = [1e-2, 0.5, 0.0]
OFFSET = [0, 1000, 3]
KEYS = [synth._fnv1a64("augment/noise_key/0/0"), (1 << 64) - 1, 5]
GARBAGE = 123.456


def _dev(a, dtype=None):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    t = torch.from_numpy(a).cuda()
    return t if dtype is None else t.to(dtype)


def _case(atoms):
    """-> (coords (3, 9, atoms, 3) f32, mask (3, 9)) on the host: non-zero garbage in the padding, a -0.0 in a valid residue of the
    sigma-0 row and one in the padding of row 1."""
    coords, mask, _ = synth.synth_batch(LENS, first_index=40)
    coords = np.ascontiguousarray(coords[:, :, :atoms])
    coords[mask == 0] = GARBAGE
    coords[2, 1, 2, 0] = -0.0
    coords[1, 5, 0, 1] = -0.0
    return coords, mask


def _tables():
    return (_dev(np.array(SIGMA, dtype=np.float32)), _dev(np.array(KEYS, dtype=np.uint64)), _dev(np.array(OFFSET, dtype=np.int32)))


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _tolerance(coords, sigma):
    """Per element 1e-5 * sigma + 2^-23 * |coord|.  |z| <= 5.77 for 24-bit uniforms; the f32 logf / sqrtf / cosine roundings add about 1e-6
    relative, a few 1e-6 in all (a numpy-f32 restatement of the generator is 1.7e-6 from the f64 one: the margin is 6x); the second term
    is the one rounding of the final add."""
    return 1e-5 * np.asarray(sigma, dtype=np.float64)[:, None, None, None] + 2.0 ** -23 * np.abs(coords.astype(np.float64))


def _check_against_reference(out, coords, streams, sigma=SIGMA, offset=OFFSET, lens=LENS):
    out = out.cpu().numpy()
    for b, n in enumerate(lens):
        ref = noise_reference(coords[b], n, sigma[b], streams[b], offset[b])
        err = np.abs(out[b].astype(np.float64) - ref.astype(np.float64))
        tol = _tolerance(coords[b:b + 1], sigma[b:b + 1])[0]
        print(f"row {b}: sigma {sigma[b]} max err {np.nanmax(err[:n]) if n else 0:.3e} (bound at sigma: {1e-5 * sigma[b]:.1e})")
        ok = (err <= tol) | (np.isnan(out[b]) & np.isnan(ref))
        assert ok.all(), (b, float(np.nanmax(err - tol)))
        if sigma[b] > 0:                      # the noise is there: the valid residues moved by about sigma
            moved = np.abs(out[b, :n].astype(np.float64) - coords[b, :n])
            assert np.nanmax(moved) > 0.5 * sigma[b] and np.nanmean(moved) < 2 * sigma[b]


@pytest.mark.parametrize("atoms", [7, 6])
def test_device_noise_matches_the_numpy_restatement(atoms):
    coords, mask = _case(atoms)
    coords[0, 3, 1, 2] = np.nan                                   # one NaN coordinate of a valid, noised residue
    c, m = _dev(coords), _dev(mask)
    sg, key, off = _tables()
    out = augment_coords(c, m, sg, key, off)
    assert out.data_ptr() != c.data_ptr() and torch.equal(_bits(c), _bits(torch.from_numpy(coords)))      # the input is const
    _check_against_reference(out, coords, KEYS)
    o = out.cpu().numpy()
    # the NaN stays NaN, its neighbours (the other two axes, the next atom) are noised
    assert np.isnan(o[0, 3, 1, 2]) and np.isnan(o).sum() == 1
    assert o[0, 3, 1, 0] != coords[0, 3, 1, 0] and o[0, 3, 1, 1] != coords[0, 3, 1, 1] and o[0, 3, 2, 0] != coords[0, 3, 2, 0]
    # the sigma-0 row and every padded residue: the input's bits (-0.0 and the garbage included)
    ob, cb = _bits(out).numpy(), _bits(torch.from_numpy(coords)).numpy()
    assert np.array_equal(ob[2], cb[2]) and ob[2, 1, 2, 0] == np.int32(-2 ** 31)
    for b, n in enumerate(LENS):
        assert np.array_equal(ob[b, n:], cb[b, n:])
    assert ob[1, 5, 0, 1] == np.int32(-2 ** 31) and o[0 + 1, 3, 0, 0] == np.float32(GARBAGE)


@pytest.mark.parametrize("atoms", [7, 6])
def test_in_place_repeatable_and_row_local(atoms):
    coords, mask = _case(atoms)
    c, m = _dev(coords), _dev(mask)
    sg, key, off = _tables()
    out = augment_coords(c, m, sg, key, off)
    again = augment_coords(c, m, sg, key, off)
    assert torch.equal(_bits(out), _bits(again))                                  # two calls: identical bytes
    inplace = c.clone()
    ret = augment_coords(inplace, m, sg, key, off, out=inplace)
    assert ret is inplace and torch.equal(_bits(inplace), _bits(out))            # in place == out of place
    keys2 = list(KEYS); keys2[0] ^= 1
    other = augment_coords(c, m, sg, _dev(np.array(keys2, dtype=np.uint64)), off)
    assert torch.equal(_bits(other[1:]), _bits(out[1:])) and not torch.equal(_bits(other[0]), _bits(out[0]))      # one key: that row only
    into = torch.full_like(c, 7.0)
    assert augment_coords(c, m, sg, key, off, out=into) is into and torch.equal(_bits(into), _bits(out))


@pytest.mark.parametrize("atoms", [7, 6])
def test_a_sample_is_independent_of_the_batch_it_lands_in(atoms):
    rna = np.ascontiguousarray(synth.synth_rna(9, 77)[:, :atoms])
    other = np.ascontiguousarray(synth.synth_rna(12, 78)[:, :atoms])
    key, sigma, offset = KEYS[0], 0.25, 17

    def place(B, T, b):
        coords = np.full((B, T, atoms, 3), GARBAGE, dtype=np.float32)
        mask = np.zeros((B, T), dtype=np.float32)
        lens = [T] * B
        lens[b] = 9
        for r in range(B):
            coords[r, :lens[r]] = rna if r == b else other[:lens[r]]
            mask[r, :lens[r]] = 1
        sg = np.full(B, 0.5, dtype=np.float32); sg[b] = sigma
        ks = np.arange(100, 100 + B, dtype=np.uint64); ks[b] = key
        of = np.arange(B, dtype=np.int32); of[b] = offset
        return augment_coords(_dev(coords), _dev(mask), _dev(sg), _dev(ks), _dev(of))[b, :9]

    first, second = place(2, 9, 0), place(3, 12, 2)
    assert torch.equal(_bits(first), _bits(second))
    assert not torch.equal(first.cpu(), torch.from_numpy(rna))
    # a slice with offset = s is rows s.. of the whole noised RNA
    whole = augment_coords(_dev(rna[None]), _dev(np.ones((1, 9), np.float32)), _dev(np.array([sigma], np.float32)),
                           _dev(np.array([key], np.uint64)), _dev(np.array([0], np.int32)))[0]
    for s in (1, 4):
        part = augment_coords(_dev(np.ascontiguousarray(rna[None, s:])), _dev(np.ones((1, 9 - s), np.float32)),
                              _dev(np.array([sigma], np.float32)), _dev(np.array([key], np.uint64)), _dev(np.array([s], np.int32)))[0]
        assert torch.equal(_bits(part), _bits(whole[s:]))


def test_without_keys_rows_draw_from_the_seed_and_row_mix():
    coords, mask = _case(7)
    c, m = _dev(coords), _dev(mask)
    sg = _dev(np.array(SIGMA, dtype=np.float32))
    seed = (7 << 40) + 12345
    out = augment_coords(c, m, sg, seed=seed)                     # key None, offset None
    _check_against_reference(out, coords, [row_stream(seed, b) for b in range(3)], offset=[0, 0, 0])
    other = augment_coords(c, m, sg, seed=seed + 1)
    assert not torch.equal(_bits(other[0]), _bits(out[0])) and not torch.equal(_bits(other[1]), _bits(out[1]))
    assert torch.equal(_bits(other[2]), _bits(out[2]))            # sigma 0
    assert len({row_stream(seed, b) for b in range(3)} | {row_stream(seed + 1, b) for b in range(3)}) == 6


def test_bad_arguments_raise():
    coords, mask = _case(7)
    sg, key, off = _tables()
    five = _dev(np.ascontiguousarray(coords[:, :, :5]))
    with pytest.raises(ValueError, match="atoms"):
        augment_coords(five, _dev(mask), sg, key, off)             # RNAMPNN_ERR_BAD_ARG
    with pytest.raises(ValueError):
        augment_coords(_dev(coords), _dev(mask), sg[:2], key, off)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        augment_coords(torch.from_numpy(coords), torch.from_numpy(mask), torch.tensor(SIGMA))


# ---------------------------------------------------------------------------------------------------------------- the main model's trainer
RNA_LENS = [12, 40, 25, 18, 33, 16, 29, 21]


def _items(atoms=7):
    return [(np.ascontiguousarray(synth.synth_rna(n, 200 + i, seed=4)[:, :atoms]), synth.synth_labels(n, 200 + i, seed=4))
            for i, n in enumerate(RNA_LENS)]


def _main_model():
    from rnampnn.model.rnampnn import RNAMPNN
    model = RNAMPNN(precision="f32", num_res_neighbours=6, num_res_mpnn_layers=2, padding_len=64)
    sd = synth.closed_form_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()})
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return model.to("cuda:0").train()


def _record_steps(trainer, model, positional):
    """Wrap ``trainer.step`` so that every step leaves (coords the step saw, loss, flat gradient, seed) behind - device clones, no sync."""
    seen, inner = [], trainer.step

    def step(*args, **kw):
        loss = inner(*args, **kw)
        seen.append((args[positional].clone(), loss.clone(), model.flat_grad.clone(), kw["seed"]))
        return loss
    trainer.step = step
    return seen


def test_main_trainer_epoch_over_augmented_items():
    from rnampnn.utils.data import pad_batch
    from rnampnn.utils.train import Trainer, plan_epoch
    items = _items()
    aug = AugmentedItems(items, noise=4, slices=4, min_len=10, noise_std=0.05, seed=2)
    lens = [int(n) for n in aug.lengths]
    model = _main_model()
    (opt,), _ = model.configure_optimizers(fused=True)
    opt.param_groups[0]["lr"] = 0.0                               # the weights stay as they are: every step can be redone afterwards
    tr = Trainer(model, opt, None, seed=3)
    seen = _record_steps(tr, model, positional=1)
    rec = tr.run_epoch(aug, lens, 0, 4, 256)
    plan, _ = plan_epoch(lens, 0, 1, 4, 256, 3)
    assert np.isfinite(rec["train_loss"]) and rec["nt"] == sum(lens) and rec["steps"] == len(plan) == len(seen) >= 4
    noisy_steps = 0
    for it, b in enumerate(plan):
        y, c, m, _ = pad_batch([aug[i] for i in b], pin=False)
        y, c, m = y.cuda(), c.cuda(), m.cuda()
        sg, key, off = _dev(aug.sigma[b]), _dev(aug.key[b]), _dev(aug.offset[b])
        manual = augment_coords(c, m, sg, key, off)
        c_seen, loss_seen, grad_seen, seed = seen[it]
        assert torch.equal(_bits(manual), _bits(c_seen))
        noisy_steps += int(not torch.equal(_bits(manual), _bits(c)))
        loss = model.loss_and_grad(y, manual, m, seed=seed)
        assert torch.equal(_bits(loss), _bits(loss_seen)) and torch.equal(_bits(model.flat_grad), _bits(grad_seen))
    assert noisy_steps >= 1


def test_epoch_over_items_wrapped_with_nothing_enabled_is_the_plain_epoch():
    from rnampnn.utils.train import Trainer
    items = _items()
    out = []
    for wrap in (False, True):
        model = _main_model()
        (opt,), (sched,) = model.configure_optimizers(fused=True)
        tr = Trainer(model, opt, sched, seed=3)
        its = AugmentedItems(items) if wrap else items
        assert EpochNoise.of(its, [[0]], "cuda") is None
        rec = tr.run_epoch(its, RNA_LENS, 0, 4, 256)
        out.append((rec, {k: v.detach().clone() for k, v in model.state_dict().items()}))
    (ra, sa), (rb, sb) = out
    assert ra["train_loss"] == rb["train_loss"] and ra["nt"] == rb["nt"] == sum(RNA_LENS) and ra["steps"] == rb["steps"]
    assert all(torch.equal(_bits(sa[k]), _bits(sb[k])) for k in sa)


# ---------------------------------------------------------------------------------------------------------------- rdesign
def _rdesign_pair(eps):
    from rdesign.model.rdesign import RNAModel
    torch.manual_seed(11)
    kw = dict(k_neighbors=6, num_mpnn_layers=2, precision="f32")
    noisy = RNAModel(augment_eps=eps, **kw)
    plain = RNAModel(**kw)
    plain.load_state_dict(noisy.state_dict())
    return noisy.cuda(), plain.cuda()


def _rdesign_batch():
    from rnampnn.utils.data import pad_batch
    S, X, mask, lens = pad_batch(_items(6), pin=False, atoms=6)
    return X.cuda(), S.cuda(), mask.cuda(), lens


def test_rdesign_augment_eps_step():
    noisy, plain = _rdesign_pair(0.05)
    X, S, mask, lens = _rdesign_batch()
    noisy.train(); plain.train()
    seed = 17
    l1 = noisy.loss_and_grad(X, S, mask, seed=seed); g1 = noisy.flat_grad.clone()
    l2 = noisy.loss_and_grad(X, S, mask, seed=seed)
    assert torch.equal(_bits(l1), _bits(l2)) and torch.equal(_bits(g1), _bits(noisy.flat_grad)) and bool(torch.isfinite(l1))
    l0 = plain.loss_and_grad(X, S, mask, seed=seed)
    assert not torch.equal(_bits(g1), _bits(plain.flat_grad)) and float(l0) != float(l1)
    sigma = torch.full((X.shape[0],), 0.05, dtype=torch.float32, device="cuda")
    Xa = augment_coords(X, mask, sigma, seed=seed)
    la = plain.loss_and_grad(Xa, S, mask, seed=seed)
    assert torch.equal(_bits(la), _bits(l1)) and torch.equal(_bits(plain.flat_grad), _bits(g1))
    l3 = noisy.loss_and_grad(X, S, mask, seed=seed + 1)          # fresh noise (and masks) with the next seed
    assert float(l3) != float(l1)
    noisy.manual_seed(seed)                                       # training_step draws the same seed from the module's counter
    with torch.no_grad():
        lt = noisy.training_step((X, S, mask, lens, None))
    assert torch.equal(_bits(lt), _bits(l1))


def test_rdesign_eval_ignores_augment_eps_and_checkpoints_keep_it(tmp_path):
    from rdesign.utils.train import load_checkpoint, save_checkpoint
    noisy, plain = _rdesign_pair(0.05)
    X, S, mask, lens = _rdesign_batch()
    noisy.eval(); plain.eval()
    assert torch.equal(_bits(noisy.forward_logits(X, mask)), _bits(plain.forward_logits(X, mask)))
    la, lb = noisy.loss_and_grad(X, S, mask, seed=3), plain.loss_and_grad(X, S, mask, seed=3)       # eval mode: p = 0, no noise
    assert torch.equal(_bits(la), _bits(lb)) and torch.equal(_bits(noisy.flat_grad), _bits(plain.flat_grad))
    path = str(tmp_path / "Final.pt")
    save_checkpoint(path, noisy)
    back, ck = load_checkpoint(path)
    assert back.augment_eps == 0.05 and ck["init_kwargs"]["augment_eps"] == 0.05
    save_checkpoint(path, plain)
    assert load_checkpoint(path)[0].augment_eps == 0.0


def test_rdesign_trainer_epoch_over_augmented_items():
    from rdesign.utils.data import padded_loader
    from rdesign.utils.train import Trainer
    items = _items(7)                                             # 7-atom records: the loader keeps six, the noise is addressed on six
    aug = AugmentedItems(items, noise=4, slices=4, min_len=10, noise_std=0.05, seed=2)
    lens = [int(n) for n in aug.lengths]
    model, _ = _rdesign_pair(0.0)
    (opt,), _ = model.configure_optimizers(fused=True)
    opt.param_groups[0]["lr"] = 0.0
    tr = Trainer(model, opt, None, seed=5)
    seen = _record_steps(tr, model, positional=1)
    rec = tr.run_epoch(aug, lens, 0, 4, 256)
    plan = tr.plan(lens, 0, 4, 256)
    assert np.isfinite(rec["train_loss"]) and rec["nt"] == sum(lens) and rec["steps"] == len(plan) == len(seen) >= 4
    noisy_steps = 0
    for it, (S, X, mask, _, b) in enumerate(padded_loader(aug, plan, device="cuda")):
        manual = augment_coords(X, mask, _dev(aug.sigma[b]), _dev(aug.key[b]), _dev(aug.offset[b]))
        X_seen, loss_seen, grad_seen, seed = seen[it]
        assert X.shape[2] == 6 and torch.equal(_bits(manual), _bits(X_seen))
        noisy_steps += int(not torch.equal(_bits(manual), _bits(X)))
        loss = model.loss_and_grad(manual, S, mask, seed=seed)
        assert torch.equal(_bits(loss), _bits(loss_seen)) and torch.equal(_bits(model.flat_grad), _bits(grad_seen))
    assert noisy_steps >= 1
