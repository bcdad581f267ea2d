"""The device's deal -- Table<N>::deal_cards of pk_device.hpp: the Philox blocks of STREAM_DECK, the chained bounded draws, the Lehmer decode on packed
bytes (with its lone last byte where 5 + 2 N = 4 k + 1) and the index -> Card.value map -- compiled for the CPU (tools/host_sim/deal_sim.cpp on
hip_shim.h) at every seat count 2 .. 16, against oracle/rng_spec.py on a few thousand (seed, table id, hand serial) triples: random ones, table ids
at both ends of the 32-bit range, hand serials on both sides of 2^32 (the serial's high word is a Philox counter word of its own).  No GPU."""
import os
import random
import shutil
import subprocess

import pytest

from oracle import rng_spec as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEATS = range(2, 17)
KMAX = 5 + 2 * 16


def triples():
    rnd = random.Random(0x6465616C)
    out = []
    edge_ids = [0, 1, 2, 0x7fffffff, 0x80000000, 0xfffffffe, 0xffffffff, 0xffffff9c]
    edge_serials = [0, 1, 17, (1 << 32) - 2, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 33) - 1, 1 << 33, (1 << 35) - 5, (1 << 63) + 3, (1 << 64) - 1]
    edge_seeds = [0, 1, 0xffffffff, 1 << 32, (1 << 64) - 1, 0x706F6B65726C]
    for tid in edge_ids:
        for hs in edge_serials:
            out.append((rnd.choice(edge_seeds), tid, hs))
    for _ in range(1200):      # ids near 2^32 with serials that cross 2^32 while a table plays on
        out.append((rnd.getrandbits(64), (0xffffffff - rnd.randrange(64)) & 0xffffffff, (1 << 32) - 32 + rnd.randrange(64)))
    for _ in range(1800):
        out.append((rnd.getrandbits(rnd.choice((16, 32, 64))), rnd.getrandbits(32), rnd.getrandbits(rnd.choice((8, 31, 33, 64)))))
    return out


@pytest.fixture(scope="module")
def decks(tmp_path_factory):
    """{(triple index, N): hex string of the deck's first 5 + 2 N Card.values} as the CPU build of deal_cards gives them"""
    if not shutil.which("g++"):
        pytest.fail("g++ not found: the CPU build of deal_cards needs it")
    exe = str(tmp_path_factory.mktemp("deal_sim") / "deal_sim")
    r = subprocess.run(["g++", "-std=c++20", "-O1", "-DPK_HOST_SIM", "-include", os.path.join(ROOT, "tools", "host_sim", "hip_shim.h"),
                        os.path.join(ROOT, "tools", "host_sim", "deal_sim.cpp"), "-o", exe], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    tr = triples()
    text = "".join("%d %d %d\n" % t for t in tr)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(tr) * len(SEATS)
    got = {}
    for i, line in enumerate(lines):
        n, hexs = line.split()
        assert int(n) == SEATS[i % len(SEATS)]
        got[(i // len(SEATS), int(n))] = hexs
    return tr, got


@pytest.fixture(scope="module")
def spec_decks():
    """per triple: Card.value of the deck's first 37 cards by the RNG spec (card i depends on the draws 0 .. i only: one list serves every seat count)"""
    canon = R.canonical_deck_values()
    return [[canon[k] for k in R.deck_permutation(seed, tid, hs, KMAX)[:KMAX]] for seed, tid, hs in triples()]


def test_triples_cover_the_edges():
    tr = triples()
    assert len(tr) >= 3000
    assert any(t[1] == 0xffffffff for t in tr) and any(t[1] == 0 for t in tr)
    assert any(t[2] < (1 << 32) for t in tr) and any(t[2] == (1 << 32) - 1 for t in tr) and any(t[2] == (1 << 32) for t in tr) and any(t[2] >> 63 for t in tr)


@pytest.mark.parametrize("n", list(SEATS))
def test_deal_cards_matches_the_rng_spec(decks, spec_decks, n):
    tr, got = decks
    k = 5 + 2 * n
    bad = []
    for i, want in enumerate(spec_decks):
        w = "".join("%02x" % v for v in want[:k])
        if got[(i, n)] != w:
            bad.append((tr[i], got[(i, n)], w))
    assert not bad, (len(bad), bad[:3])


def test_a_deck_has_no_card_twice(decks):
    tr, got = decks
    for (i, n), hexs in got.items():
        vals = [int(hexs[2 * j:2 * j + 2], 16) for j in range(5 + 2 * n)]
        assert len(set(vals)) == len(vals) and all((v & 0xf) < 13 and (v >> 4) < 4 for v in vals), (tr[i], n, hexs)
