"""CPU tests of the table snapshots (no GPU): the blob size, argument refusals that need no device, the new kernels in the built
library's code objects, and the Python restatement of the clone's redeal."""
import os
import re
import sys

import numpy as np
import pytest

import snapshot_spec as SS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SNAP_KERNELS = ("k_snap_save", "k_snap_check", "k_snap_check_idx", "k_snap_load", "k_snap_clone")


@pytest.fixture(scope="module")
def lib():
    from pokerl_amd import _lib, build
    build.build_lib()
    return _lib


def test_snapshot_bytes_formula(lib):
    import pokerl_amd
    for n in range(lib.MIN_PLAYERS, lib.MAX_PLAYERS + 1):
        for m in (0, 1, 7, 64, 1000, 65536, 1048576):
            assert lib.lib().pk_snapshot_bytes(n, m) == pokerl_amd.snapshot_nbytes(n, m) == SS.nbytes(n, m), (n, m)
    assert pokerl_amd.snapshot_nbytes(6, 1048576) // 1048576 == 278       # 278 B per table and direction at six seats
    for n in (-1, 0, 1, 17, 23):
        assert lib.lib().pk_snapshot_bytes(n, 10) == 0


def test_null_handle_or_blob_is_refused_without_a_device(lib):
    L = lib.lib()
    for fn in (L.pk_save_tables_d, L.pk_load_tables_d, L.pk_save_tables, L.pk_load_tables):
        assert fn(None, None, 4, None) == lib.PK_E_INVALID_ARG
    assert L.pk_clone_tables_d(None, None, None, None, 4, -1, 0) == lib.PK_E_INVALID_ARG


def test_snapshot_kernels_exist_without_scratch(lib):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    ks = kernel_meta.kernels(lib.LIB_PATH)
    for k in SNAP_KERNELS:
        assert k in ks, k
        assert ks[k]["private_segment"] == 0, (k, ks[k])
        assert not re.match(r"k_(reset|make_fresh|pick|rollout|step|env_)", k)


@pytest.mark.parametrize("n", [2, 6, 9, 16])
def test_redeal_restatement_keeps_visible_cards_and_permutes(n):
    from oracle import rng_spec as R
    rng = np.random.default_rng(n)
    for trial in range(40):
        deck = np.array([R.canonical_deck_values()[k] for k in rng.permutation(52)[:5 + 2 * n]], np.uint8)
        turn, p = int(rng.integers(0, 5)), int(rng.integers(0, n))
        out = SS.redeal(deck, n, turn, p, seed=12345 + trial, table_id=trial, nonce=trial * 7)
        nb, vis = SS.visible_positions(n, turn, p)
        assert all(out[i] == deck[i] for i in vis)
        assert len(set(out.tolist())) == 5 + 2 * n                     # distinct cards
        assert all(((v >> 4) < 4) and ((v & 15) < 13) for v in out)    # every byte a card
        hidden_in = set(out.tolist()) - {int(deck[i]) for i in vis}
        assert not hidden_in & {int(deck[i]) for i in vis}


def test_table_indices_outside_int32_are_refused_before_the_cast():
    from pokerl_amd.game import VecGame
    g = VecGame.__new__(VecGame)                    # the index conversion needs no handle
    for bad in ([2 ** 32 + 5], [-2 ** 31 - 1], np.array([0, 2 ** 40], np.int64)):
        with pytest.raises(IndexError):
            g._tables(bad)
    with pytest.raises(TypeError):
        g._tables([1.0])
    assert g._tables(np.array([0, 2 ** 31 - 1], np.int64)).dtype == np.int32
