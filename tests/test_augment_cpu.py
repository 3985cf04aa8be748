"""CPU checks of the training-set augmentations (``rnampnn/utils/augment.py``): the quality of the counter generator the noise is drawn
from, the table of virtual samples ``AugmentedItems`` builds, the epoch plan over it, the C ABI symbol and the CLI defaults.  What the
device kernel computes is checked against ``noise_reference`` in ``test_augment_gpu.py``."""
import numpy as np
import pytest

from rnampnn.utils import synth
from rnampnn.utils.augment import AugmentedItems, noise_reference

N_VALUES = 64 * 100 * 21                  # 134,400 values per stream: a (64, 100, 7, 3) batch
KEYS = [0, 1, (1 << 64) - 1, synth._fnv1a64("augment/noise_key/0/0"), synth._fnv1a64("augment/noise_key/0/1")]


@pytest.fixture(scope="module")
def streams():
    """key -> N_VALUES normals, for every key of KEYS and its successor (computed once)."""
    idx = np.arange(N_VALUES, dtype=np.uint64)
    return {k: synth.normal01(k, idx) for key in KEYS for k in (key, (key + 1) & ((1 << 64) - 1))}


@pytest.mark.parametrize("key", KEYS)
def test_generator_moments_and_independence(streams, key):
    """Each statistic is scaled by its standard error for i.i.d. N(0, 1) values (mean: 1/sqrt(N); variance: sqrt(2/N); a product of two
    independent normals has variance 1, so both covariances: 1/sqrt(N)); 5 standard errors."""
    z, z1 = streams[key], streams[(key + 1) & ((1 << 64) - 1)]
    n = float(N_VALUES)
    stats = dict(mean=abs(z.mean()) * np.sqrt(n), var=abs(z.var() - 1.0) * np.sqrt(n / 2), lag1=abs(np.mean(z[:-1] * z[1:])) * np.sqrt(n),
                 next_key=abs(np.mean(z * z1)) * np.sqrt(n))
    print(key, stats)
    assert np.isfinite(z).all() and np.abs(z).max() <= 5.77         # sqrt(-2 ln 2^-24) = 5.768
    for name, v in stats.items():
        assert v < 5, (name, v)


def test_noise_reference_is_the_generator_on_the_stated_index():
    c = synth.synth_rna(9, 3)                                       # (9, 7, 3)
    out = noise_reference(c, 4, 0.5, 77, offset=1000)
    z = synth.normal01(77, np.arange(4 * 21, dtype=np.uint64) + np.uint64(1000 * 21)).reshape(4, 7, 3)
    assert np.array_equal(out[:4], c[:4] + (0.5 * z).astype(np.float32)) and out.dtype == np.float32
    assert np.array_equal(out[4:].view(np.int32), c[4:].view(np.int32))
    assert np.array_equal(noise_reference(c, 9, 0.0, 77).view(np.int32), c.view(np.int32))
    six = noise_reference(c[:, :6], 9, 0.5, 77)                     # six atoms: 18 values per residue, another addressing
    z6 = synth.normal01(77, np.arange(9 * 18, dtype=np.uint64)).reshape(9, 6, 3)
    assert np.array_equal(six, c[:, :6] + (0.5 * z6).astype(np.float32))
    whole = noise_reference(c, 9, 0.5, 77)                          # a slice at offset s carries rows s.. of the whole RNA's noise
    assert np.array_equal(noise_reference(c[3:], 6, 0.5, 77, offset=3), whole[3:])


# ------------------------------------------------------------------------------------------------------------------ AugmentedItems
LENGTHS = [12, 40, 25, 18, 33, 9, 29, 21]


def _items(with_id=False):
    out = []
    for i, n in enumerate(LENGTHS):
        c, y = synth.synth_rna(n, i, seed=2), synth.synth_labels(n, i, seed=2)
        out.append((f"rna{i}", c, y) if with_id else (c, y))
    return out


@pytest.mark.parametrize("with_id", [False, True])
def test_augmented_items_table(with_id):
    items = _items(with_id)
    n0, n_noise, n_slice, min_len = len(items), 6, 200, 20
    aug = AugmentedItems(items, noise=n_noise, slices=n_slice, min_len=min_len, noise_std=0.03, seed=5)
    assert len(aug) == n0 + n_noise + n_slice and aug.augments
    for name, dt in (("lengths", np.int64), ("source", np.int64), ("sigma", np.float32), ("key", np.uint64), ("offset", np.int32)):
        a = getattr(aug, name)
        assert a.shape == (len(aug),) and a.dtype == dt, name
    # originals first, untouched
    assert aug.lengths[:n0].tolist() == LENGTHS and aug.source[:n0].tolist() == list(range(n0))
    assert not aug.sigma[:n0].any() and not aug.offset[:n0].any()
    assert all(aug[i] is items[i] for i in range(n0))
    # noisy copies: whole RNAs among the originals, sigma = noise_std, distinct keys
    cp = slice(n0, n0 + n_noise)
    assert ((0 <= aug.source[cp]) & (aug.source[cp] < n0)).all()
    assert aug.lengths[cp].tolist() == [LENGTHS[s] for s in aug.source[cp]]
    assert (aug.sigma[cp] == np.float32(0.03)).all() and not aug.offset[cp].any()
    assert len(set(aug.key[cp].tolist())) == n_noise
    # slices
    sl = slice(n0 + n_noise, len(aug))
    src_len = np.array(LENGTHS)[aug.source[sl]]
    assert (aug.lengths[sl] == min_len).all() and (src_len > min_len).all()
    assert (aug.offset[sl] >= 0).all() and (aug.offset[sl] <= src_len - min_len).all()
    assert len(set(aug.offset[sl].tolist())) > 1 and (aug.offset[sl] == src_len - min_len).any() and (aug.offset[sl] == 0).any()
    copy_of_key = {int(k): j for j, k in zip(range(n0, n0 + n_noise), aug.key[cp])}
    from_copy = 0
    for i in range(n0 + n_noise, len(aug)):
        if aug.sigma[i] > 0:                          # a slice of a noisy copy: that copy's key, sigma and source, offset = its start
            j = copy_of_key[int(aug.key[i])]
            assert aug.sigma[i] == aug.sigma[j] and aug.source[i] == aug.source[j]
            from_copy += 1
        else:
            assert aug.key[i] == 0
        it, src = aug[i], items[int(aug.source[i])]
        assert len(it) == len(src)
        c, y = it[-2], it[-1]
        s = int(aug.offset[i])
        assert c.shape == (min_len, 7, 3) and y.shape == (min_len,)
        assert np.shares_memory(c, src[-2]) and np.shares_memory(y, src[-1])
        assert np.array_equal(c, src[-2][s:s + min_len]) and np.array_equal(y, src[-1][s:s + min_len])
        if with_id:
            assert it[0] == src[0]
    assert 0 < from_copy < n_slice                    # both kinds of source were drawn
    for i in range(n0, n0 + n_noise):                 # a noisy copy is the source's arrays (the noise lives in the table)
        assert np.shares_memory(aug[i][-2], items[int(aug.source[i])][-2])
    assert aug[-1] is aug[len(aug) - 1] or np.shares_memory(aug[-1][-2], aug[len(aug) - 1][-2])
    with pytest.raises(IndexError):
        aug[len(aug)]
    with pytest.raises(ValueError):                   # read-only table
        aug.sigma[0] = 1.0


def test_augmented_items_depend_on_the_seed_alone():
    items = _items()
    tab = lambda a: [getattr(a, n).tolist() for n in ("lengths", "source", "sigma", "key", "offset")]
    a, b = (AugmentedItems(items, noise=16, slices=16, min_len=15, seed=9) for _ in range(2))
    c = AugmentedItems(items, noise=16, slices=16, min_len=15, seed=10)
    assert tab(a) == tab(b)
    assert a.source.tolist() != c.source.tolist() and a.offset.tolist() != c.offset.tolist()
    assert not set(a.key[8:24].tolist()) & set(c.key[8:24].tolist())
    state = np.random.get_state()[1].copy()
    AugmentedItems(items, noise=4, slices=4, min_len=15, seed=1)
    assert np.array_equal(np.random.get_state()[1], state)          # no global RNG state is consumed


def test_nothing_long_enough_raises_as_the_reference_does():
    with pytest.raises(ValueError, match="longer than min_len"):
        AugmentedItems(_items(), noise=3, slices=1, min_len=40)      # the longest RNA has 40 residues: none is LONGER
    AugmentedItems(_items(), noise=3, slices=1, min_len=39)


def test_identity_without_augmentation():
    items = _items(True)
    aug = AugmentedItems(items)
    assert len(aug) == len(items) and not aug.augments
    assert all(aug[i] is items[i] for i in range(len(items)))
    assert aug.lengths.tolist() == LENGTHS and not aug.sigma.any()
    sl = AugmentedItems(items, slices=5, min_len=10)                 # slices of plain RNAs carry no noise
    assert not sl.augments and len(sl) == len(items) + 5


def test_plan_epoch_visits_every_virtual_sample():
    from rnampnn.utils.train import plan_epoch
    aug = AugmentedItems(_items(), noise=7, slices=9, min_len=10, seed=3)
    for world in (1, 2):
        seen = []
        for rank in range(world):
            mine, _ = plan_epoch(aug.lengths, rank, world, 4, 96, seed=11)
            assert all(len(b) * max(int(aug.lengths[i]) for i in b) <= 96 for b in mine)
            seen += [i for b in mine for i in b]
        assert set(seen) == set(range(len(aug)))


def test_header_declares_and_library_exports_the_symbol():
    import __graft_entry__ as g
    g.build()
    from rnampnn import _native
    lib = _native.lib()
    assert hasattr(lib, "rnampnn_augment_coords") and "rnampnn_augment_coords" in _native.SYMBOLS
    assert "augment.hip" in g.SOURCES


def test_cli_defaults_leave_augmentation_off():
    import os
    import sys
    from conftest import REPO
    sys.path.insert(0, os.path.join(REPO, "rna-mpnn_amd"))
    import train
    a = train.parse([])
    assert (a.noise_augmentation, a.slice_augmentation, a.slice_len, a.noise_std, a.augment_eps) == (0, 0, 1000, 1e-2, 0.0)
    items = _items()
    same, lens = train._augment(items, LENGTHS, a)
    assert same is items and lens is LENGTHS                         # today's path: the plain list
    b = train.parse(["--noise-augmentation", "5", "--slice-augmentation", "3", "--slice-len", "20", "--noise-std", "0.02", "--seed", "4"])
    aug, lens = train._augment(items, LENGTHS, b)
    assert isinstance(aug, AugmentedItems) and len(aug) == len(items) + 8 and lens == aug.lengths.tolist()
    assert (aug.sigma[8:13] == np.float32(0.02)).all() and (aug.lengths[13:] == 20).all()


def test_rdesign_model_keeps_augment_eps_in_its_constructor_arguments():
    from rdesign.model.rdesign import RNAModel
    m = RNAModel(num_mpnn_layers=1, precision="f32", augment_eps=0.05)
    assert m.init_kwargs["augment_eps"] == 0.05 and RNAModel(**m.init_kwargs).augment_eps == 0.05
    assert RNAModel(num_mpnn_layers=1, precision="f32").init_kwargs["augment_eps"] == 0.0
    with pytest.raises(ValueError):
        RNAModel(num_mpnn_layers=1, precision="f32", augment_eps=-1.0)
