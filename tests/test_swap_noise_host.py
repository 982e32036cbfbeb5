"""Swap noise on the host: InputNoise("swap") validation, the config block, the numpy statement of apply and swapped() against the
plain-Python loop of tests/swap_ref.py, and what the draw is keyed by.  No GPU."""
import re
import os

import numpy as np
import pytest
import torch

import swap_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _noise(fx, seed=R.SEED, pool=True):
    from codae.tool import InputNoise
    return InputNoise("swap", p=fx["p"], seed=seed, pool=fx["pool"] if pool else None)


def _data(S, E, seed=3):
    return np.random.default_rng(seed).standard_normal((R.N_ROWS, S * E)).astype(np.float32)


def test_validation_of_kind_p_pool_data_and_slots():
    from codae.hip import HipError
    from codae.tool import InputNoise
    n = InputNoise("swap", p=0.15, seed=3)
    assert n.kind == "swap" and n.code == 4 and n.pool is None and abs(n.p - 0.15) < 1e-7
    assert n.as_struct().kind == 4 and n.threshold == int(np.floor(float(np.float32(0.15)) * 2.0 ** 32))
    assert InputNoise("swap", p=0.5, pool=torch.tensor([3, 1, 2])).pool.tolist() == [3, 1, 2]
    assert InputNoise("swap", p=0.5, pool=[5, 5, 0]).pool.dtype == np.int64
    for bad in (dict(p=-0.1), dict(p=1.5), dict(p=None), dict(p=0.1, sigma=0.2), dict(p=0.1, lo=0.0)):
        with pytest.raises(HipError):
            InputNoise("swap", **bad)
    with pytest.raises(HipError, match="unknown kind"):
        InputNoise("swop", p=0.1)
    with pytest.raises(HipError, match="empty"):
        InputNoise("swap", p=0.1, pool=[])
    with pytest.raises(HipError, match="integer"):
        InputNoise("swap", p=0.1, pool=[0.5, 1.0])
    with pytest.raises(HipError, match=r"\[0, 2\^31\)"):
        InputNoise("swap", p=0.1, pool=[-1, 2])
    with pytest.raises(HipError, match="takes no pool"):
        InputNoise("masking", p=0.1, pool=[1])
    with pytest.raises(HipError, match="outside the dataset"):
        InputNoise("swap", p=0.1, pool=[1, 64]).pool_rows(64)
    x = torch.zeros(4, 6)
    with pytest.raises(HipError, match="needs data .* and n_slots"):
        n.apply(x, [0, 1, 2, 3], 1)
    with pytest.raises(HipError, match="needs data .* and n_slots"):
        n.apply(x, [0, 1, 2, 3], 1, data=torch.zeros(8, 6))
    with pytest.raises(HipError, match="does not divide"):
        n.apply(x, [0, 1, 2, 3], 1, data=torch.zeros(8, 6), n_slots=4)
    with pytest.raises(HipError, match="outside the dataset"):
        InputNoise("swap", p=0.1, pool=[9]).apply(x, [0, 1, 2, 3], 1, data=torch.zeros(8, 6), n_slots=2)
    with pytest.raises(HipError, match="swap noise only"):
        InputNoise("masking", p=0.1).apply(x, [0, 1, 2, 3], 1, n_slots=2)
    with pytest.raises(HipError, match="n_rows is required"):
        n.swapped([0, 1], 1, 2)
    with pytest.raises(HipError, match="swaps nothing"):
        InputNoise("masking", p=0.1).swapped([0, 1], 1, 2, n_rows=4)


def test_config_block_pool_values_and_unknown_keys():
    from codae.hip import HipError
    from codae.tool.noise import input_noise_from_config
    train = [4, 9, 2, 7]
    n = input_noise_from_config({"KIND": "swap", "P": 0.15, "SEED": 7}, train_rows=train)
    assert n.kind == "swap" and n.seed == 7 and n.pool.tolist() == train              # the default: the training rows
    assert input_noise_from_config({"KIND": "swap", "P": 0.15, "POOL": "train"}, train_rows=train).pool.tolist() == train
    assert input_noise_from_config({"KIND": "swap", "P": 0.15, "POOL": "all"}, train_rows=train).pool is None
    with pytest.raises(HipError, match="unknown POOL"):
        input_noise_from_config({"KIND": "swap", "P": 0.15, "POOL": "validation"}, train_rows=train)
    with pytest.raises(HipError, match="unknown key"):
        input_noise_from_config({"KIND": "swap", "P": 0.15, "POOLS": "all"}, train_rows=train)
    with pytest.raises(HipError, match="needs the training rows"):
        input_noise_from_config({"KIND": "swap", "P": 0.15})
    with pytest.raises(HipError, match="swap only"):
        input_noise_from_config({"KIND": "masking", "P": 0.15, "POOL": "all"})
    assert input_noise_from_config({"KIND": "masking", "P": 0.15}).kind == "masking"       # the other kinds as before


@pytest.mark.parametrize("S,E", [(3, 16), (2, 12), (11, 4)])
def test_numpy_apply_and_swapped_match_the_plain_loop(S, E):
    fx = R.fixture(S)
    data = _data(S, E)
    keep = np.ones((R.N_ROWS, S * E), dtype=np.uint8)
    for b in range(R.N_ROWS):
        keep[b, (b % S) * E:(b % S + 1) * E] = 0
    for step in (1, 2):
        ref, cls = R.corrupt(data, data, fx["rows"], step, S, fx["p"], R.SEED, fx["pool"], fx["present"], keep)
        R.assert_all_classes(cls)
        for pool in (True, False):
            for pres in (fx["present"], None):
                for mask in (keep, None):
                    n = _noise(fx, pool=pool)
                    ref, cls = R.corrupt(data, data, fx["rows"], step, S, fx["p"], R.SEED, fx["pool"] if pool else None, pres, mask)
                    _, src = R.classify(fx["rows"], step, S, fx["p"], R.SEED, R.N_ROWS, fx["pool"] if pool else None, pres)
                    acc, source = n.swapped(fx["rows"], step, S, n_rows=R.N_ROWS, presence=pres)
                    assert np.array_equal(acc, cls == 3) and np.array_equal(source, src)
                    got = n.apply(torch.tensor(data), fx["rows"], step, mask=None if mask is None else torch.tensor(mask),
                                  data=torch.tensor(data), presence=pres, n_slots=S).numpy()
                    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
                    assert (cls == 3).any() and not np.array_equal(got, data if mask is None else data * mask)
    # a SlotPresence object is taken like its table
    from codae.tool import SlotPresence
    n = _noise(fx)
    a = n.swapped(fx["rows"], 1, S, n_rows=R.N_ROWS, presence=SlotPresence(fx["present"]))[0]
    assert np.array_equal(a, n.swapped(fx["rows"], 1, S, n_rows=R.N_ROWS, presence=fx["present"])[0])


def test_fixture_counts_of_the_definition():
    """The table the definition was evaluated to: (hit, rejected as self, rejected by presence, accepted, rows without a swap)."""
    fx = R.fixture(3)
    want = {1: (75, 2, 33, 40, 32), 2: (79, 1, 46, 32, 38)}
    for step, w in want.items():
        cls, _ = R.classify(fx["rows"], step, 3, fx["p"], R.SEED, R.N_ROWS, fx["pool"], fx["present"])
        got = (int((cls != 0).sum()), int((cls == 1).sum()), int((cls == 2).sum()), int((cls == 3).sum()), int((~(cls == 3).any(1)).sum()))
        assert got == w, (step, got)


def test_the_key_is_the_dataset_row_not_the_batch_position():
    S, E = 3, 16
    fx = R.fixture(S)
    data = _data(S, E)
    n = _noise(fx)
    cls, _ = R.classify(fx["rows"], 1, S, fx["p"], R.SEED, R.N_ROWS, fx["pool"], fx["present"])
    R.assert_all_classes(cls)
    full = n.apply(torch.tensor(data), fx["rows"], 1, data=torch.tensor(data), presence=fx["present"], n_slots=S)
    perm = np.random.default_rng(5).permutation(R.N_ROWS)
    moved = n.apply(torch.tensor(data[perm]), perm, 1, data=torch.tensor(data), presence=fx["present"], n_slots=S)
    assert torch.equal(moved, full[perm])
    part = perm[:17]
    assert torch.equal(n.apply(torch.tensor(data[part]), part, 1, data=torch.tensor(data), presence=fx["present"], n_slots=S), full[part])
    acc, src = n.swapped(perm, 1, S, n_rows=R.N_ROWS, presence=fx["present"])
    acc0, src0 = n.swapped(fx["rows"], 1, S, n_rows=R.N_ROWS, presence=fx["present"])
    assert np.array_equal(acc, acc0[perm]) and np.array_equal(src, src0[perm])


def test_the_stream_differs_between_steps_seeds_key_words_and_from_masking():
    from codae.tool.noise import noise_words, swap_words
    rows, S = np.arange(R.N_ROWS), 3
    base = np.stack(swap_words(rows, S, 1, R.SEED))
    assert not np.array_equal(base, np.stack(swap_words(rows, S, 2, R.SEED)))                   # the step
    assert not np.array_equal(base, np.stack(swap_words(rows, S, 1, R.SEED + 1)))               # the seed's low word
    assert not np.array_equal(base, np.stack(swap_words(rows, S, 1, R.SEED + (1 << 32))))       # the key's high word
    assert (base != np.stack(swap_words(rows, S, 1, R.SEED + (1 << 32)))).mean() > 0.99
    # counter word 3 is 512: the masking stream of the same seed has other words at the same (group, row, step)
    mask_words = noise_words(rows, 4 * S, 1, R.SEED).reshape(R.N_ROWS, S, 4)
    assert (mask_words[:, :, 0] != base[0]).mean() > 0.99 and (mask_words[:, :, 1] != base[1]).mean() > 0.99
    w = R.draw(5, 2, 1, R.SEED)
    assert (int(base[0][5, 2]), int(base[1][5, 2])) == w
    # accepted sets of two steps / two seeds differ
    fx = R.fixture(S)
    a1 = _noise(fx).swapped(rows, 1, S, n_rows=R.N_ROWS)[0]
    assert not np.array_equal(a1, _noise(fx).swapped(rows, 2, S, n_rows=R.N_ROWS)[0])
    assert not np.array_equal(a1, _noise(fx, seed=8).swapped(rows, 1, S, n_rows=R.N_ROWS)[0])


def test_header_binding_and_documents_name_the_kind():
    from codae import hip
    header = open(os.path.join(ROOT, "include", "codae_hip.h")).read()
    assert re.search(r"CODAE_NOISE_SWAP\s*=\s*4\b", header) and hip.NOISE_SWAP == 4
    import ctypes as C
    assert C.sizeof(hip.Swap) == 16 and C.sizeof(hip.Noise) == 24                      # codae_noise keeps its layout
    for name in ("codae_set_swap_pool", "codae_corrupt_batch_swap", "codae_emph_loss_swap", "codae_recon_loss_fwd_bwd_swap"):
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, header)
        assert m and name in hip.PROTOTYPES and len(hip.PROTOTYPES[name][1]) == m.group(1).count(",") + 1, name
    for doc in ("README.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert 'InputNoise("swap"' in text and "Not covered" in text, doc
