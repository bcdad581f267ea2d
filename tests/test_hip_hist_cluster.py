"""GPU tests of the histogram clustering (pk_hist_cluster*): every output of the device against the numpy restatement tests/hist_cluster_spec.py by
exact integer equality -- quantise + assign at the smallest shapes that can go wrong, empty rows, constructed ties, the W = 0 seeding rule,
the iteration on 70 001 rows, more rows than one pass of the grid, seeding with nonces, the composition with strength_histogram_batch, the
device form on a caller's stream, and the argument errors."""
import ctypes as C

import numpy as np
import pytest

import hist_cluster_spec as CS

pytestmark = pytest.mark.gpu

SEED = 0x706F6B65726C
BLOCK, GRID_MAX, UNROLL = 256, 2048, 2            # pk_hist_cluster.hpp: CL_BLOCK, CL_GRID_MAX; k_cl_assign unrolls two centroids


@pytest.fixture(scope="module")
def PK():
    import pokerl_amd
    assert pokerl_amd.device_count() >= 1, "no MI355X visible: the HIP path cannot run (there is no fallback)"
    return pokerl_amd


def rows(seed, n, nbins, empty_frac=0.1, shapes=12):
    return CS.latent_rows(np.random.default_rng(seed), n, nbins, mass=46, shapes=shapes, empty_frac=empty_frac)


def centroids_near(seed, hist, K):
    rng = np.random.default_rng(seed)
    q, empty = CS.quant(hist)
    c = q[rng.choice(np.flatnonzero(~empty), K)].astype(np.int64)
    c[::2] = np.sort(np.clip(c[::2] + rng.integers(-700, 700, c[::2].shape), 0, 65535), axis=1)
    return c.astype(np.uint16)


def check_assign(J, hist, cen):
    q, empty = CS.quant(hist)
    want_l, want_d = CS.assign(q, empty, cen)
    label, dist = J.assign_histograms(hist, cen)
    assert label.dtype == np.uint16 and dist.dtype == np.uint32
    assert np.array_equal(label, want_l), np.flatnonzero(label != want_l)[:5]
    assert np.array_equal(dist, want_d), np.flatnonzero(dist != want_d)[:5]
    return label, dist


def check_cluster(J, hist, cen, iters):
    q, empty = CS.quant(hist)
    want = CS.iterate(q, empty, cen, iters)
    n, nbins = hist.shape
    out = cen.copy()
    label, dist = np.full(n, 7, np.uint16), np.full(n, 7, np.uint32)
    inertia, changed = np.full(iters + 1, 7, np.uint64), np.full(iters, 7, np.uint32)
    from pokerl_amd import _lib as L
    L.check(L.lib().pk_hist_cluster(0, n, nbins, L.ptr(hist), cen.shape[0], L.ptr(out), iters, L.ptr(label), L.ptr(dist), L.ptr(inertia), L.ptr(changed)))
    assert np.array_equal(changed, want["changed"]), (changed, want["changed"])
    assert np.array_equal(inertia, want["inertia"]), (inertia, want["inertia"])
    assert np.array_equal(out, want["centroids"]) and np.array_equal(label, want["labels"]) and np.array_equal(dist, want["dist"])
    assert int(dist.sum(dtype=np.uint64)) == int(inertia[-1])
    return dict(centroids=out, labels=label, dist=dist, inertia=inertia, changed=changed)


@pytest.mark.parametrize("nbins", [1, 2, 7, 10, 32])
@pytest.mark.parametrize("n", [1, 63, 64, 65, BLOCK + 1])
def test_assign_at_the_smallest_shapes(PK, n, nbins):
    from pokerl_amd import judger as J
    hist = rows(1000 * nbins + n, n, nbins, empty_frac=0.0 if n == 1 else 0.1)
    for K in (1, 2, UNROLL + 1, n + 7):                              # assign takes any K: more centroids than rows included
        check_assign(J, hist, centroids_near(K, hist, K))


@pytest.mark.parametrize("nbins", [7, 10])
def test_empty_rows_first_last_and_as_whole_waves(PK, nbins):
    from pokerl_amd import judger as J
    hist = rows(31 + nbins, 5 * 64 + 9, nbins, empty_frac=0.0)
    hist[:3] = 0
    hist[64:192] = 0                                                 # two whole waves
    hist[-2:] = 0
    label, dist = check_assign(J, hist, centroids_near(5, hist, 5))
    assert (label[64:192] == CS.NONE).all() and not dist[64:192].any() and (label[:3] == CS.NONE).all() and (label[-2:] == CS.NONE).all()
    r = check_cluster(J, hist, centroids_near(6, hist, 4), 2)
    assert r["changed"][0] == 5 * 64 + 9 - 3 - 128 - 2


def test_constructed_ties(PK):
    from pokerl_amd import judger as J
    t = np.zeros((70, 4), np.uint16)
    t[::3] = [4, 0, 0, 0]
    t[1::3] = [0, 0, 0, 4]                                           # duplicated rows
    t[2::3] = [2, 0, 0, 2]                                           # q = (32767, 32767, 32767, 65535)
    cen = np.array([[65535, 65535, 65535, 65535], [0, 0, 0, 65535], [0, 0, 0, 65535], [65534, 65535, 65535, 65535]], np.uint16)
    label, _ = check_assign(J, t, cen)
    assert set(label.tolist()) == {0, 1}                             # two identical centroids: the smaller index wins
    r = check_cluster(J, t, cen, 1)
    assert r["centroids"][2].tolist() == [0, 0, 0, 65535]            # ... and the larger stays empty and keeps its centroid
    mid = np.zeros((3, 2), np.uint16)
    mid[:] = [[1, 1], [1, 0], [0, 1]]                                # q[0] = (32767, 65535)
    label, dist = check_assign(J, mid, np.array([[32767 + 100, 65535], [32767 - 100, 65535], [32767 + 100, 65535]], np.uint16))
    assert label[0] == 0 and dist[0] == 100                          # exactly midway between centroids 0 and 1


def test_identical_rows_seed_by_the_w0_rule_and_leave_clusters_empty(PK):
    from pokerl_amd import judger as J
    hist = np.zeros((300, 10), np.uint16)
    hist[:] = [1, 0, 3, 0, 0, 9, 0, 0, 2, 1]
    hist[:70] = 0
    hist[200:264] = 0
    q, empty = CS.quant(hist)
    want, chosen = CS.seed(q, empty, 3, SEED, 2)
    assert chosen[1:] == [70, 70]
    cen = J.seed_histogram_centroids(hist, 3, seed=SEED, nonce=2)
    assert np.array_equal(cen, want) and (cen == q[70]).all()
    r = check_cluster(J, hist, cen, 2)
    assert set(r["labels"][~empty].tolist()) == {0} and not r["dist"].any() and r["changed"].tolist() == [int((~empty).sum()), 0]


def test_70001_rows_257_centroids_7_bins_three_iterations(PK):
    from pokerl_amd import judger as J
    hist = rows(70001, 70001, 7)
    assert 0.08 < (hist.sum(axis=1) == 0).mean() < 0.12
    q, empty = CS.quant(hist)
    want_seed, _ = CS.seed(q, empty, 257, SEED, 1)
    cen = J.seed_histogram_centroids(hist, 257, seed=SEED, nonce=1)
    assert np.array_equal(cen, want_seed)
    r = check_cluster(J, hist, cen, 3)                               # K * nbins <= 4096: the sums are kept in LDS
    assert r["changed"][0] == (~empty).sum() and r["changed"][2] > 0


def test_more_rows_than_one_pass_of_the_grid_and_the_global_sums(PK):
    from pokerl_amd import judger as J
    n = BLOCK * GRID_MAX + 65                                        # every workgroup strides once; the last pass is one partial workgroup
    hist = rows(5, n, 2, shapes=3)
    check_cluster(J, hist, centroids_near(8, hist, 2), 1)
    small = rows(6, 3000, 32)                                        # K * nbins > 4096: sums by global atomics
    check_cluster(J, small, centroids_near(9, small, 129), 2)


@pytest.mark.parametrize("K", [1, 2, 33])
def test_seeding_equals_the_spec_and_follows_the_nonce(PK, K):
    from pokerl_amd import judger as J
    hist = rows(77, 5000, 10)                                        # 20 chunks of one tile
    q, empty = CS.quant(hist)
    got = [J.seed_histogram_centroids(hist, K, seed=SEED + 1, nonce=nonce) for nonce in (0, 1, 0)]
    for nonce, cen in zip((0, 1, 0), got):
        assert np.array_equal(cen, CS.seed(q, empty, K, SEED + 1, nonce)[0]), nonce
    assert np.array_equal(got[0], got[2]) and not np.array_equal(got[0], got[1])
    big = rows(78, 300000, 2, shapes=4)                              # chunks of two tiles: the search inside a chunk walks on
    qb, eb = CS.quant(big)
    assert np.array_equal(J.seed_histogram_centroids(big, K, seed=9, nonce=4), CS.seed(qb, eb, K, 9, 4)[0])


def test_composition_with_strength_histograms_and_the_device_form(PK):
    from pokerl_amd import hipmem
    from pokerl_amd import judger as J
    board = np.array([[0x2C, 0x18, 0x33, 0x05, 0], [0x01, 0x12, 0x23, 0x39, 0]], np.uint8)   # two full-pool turn boards
    h = J.strength_histogram_batch(board, np.array([4, 4], np.uint8), bins=10)
    assert not h.status.any() and h.valid.sum() == 2 * 1128
    r = h.cluster(8, iters=5, seed=SEED, nonce=3)
    assert r.labels.shape == (2, 1326) and r.dist.shape == (2, 1326) and (r.k, r.bins) == (8, 10)
    assert ((r.labels == CS.NONE) == ~h.valid).all() and set(r.labels[h.valid].tolist()) <= set(range(8))
    flat = h.hist.reshape(-1, 10)
    q, empty = CS.quant(flat)
    want = CS.iterate(q, empty, CS.seed(q, empty, 8, SEED, 3)[0], 5)
    ran = len(r.changed)
    assert np.array_equal(r.centroids, want["centroids"]) and np.array_equal(r.labels.reshape(-1), want["labels"])
    assert np.array_equal(r.changed, want["changed"][:ran]) and np.array_equal(r.inertia[:ran], want["inertia"][:ran]) and r.inertia[-1] == want["inertia"][-1]
    assert int(r.dist.sum(dtype=np.uint64)) == int(r.inertia[-1]) and np.allclose(r.emd, r.dist / 65535.0)
    label, dist = r.assign(h.hist)                                   # the training rows under the learned centroids: the same labels
    assert np.array_equal(label, r.labels) and np.array_equal(dist, r.dist)
    # the device form on a caller's stream == the host form
    hip = hipmem._lib()
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0
    n = flat.shape[0]
    hist_d, cen_d = hipmem.DeviceBuffer(flat.nbytes).upload(flat), hipmem.DeviceBuffer(8 * 10 * 2).upload(np.full(80, 7, np.uint16))
    label_d, dist_d = hipmem.DeviceBuffer(n * 2).upload(np.full(n, 7, np.uint16)), hipmem.DeviceBuffer(n * 4).upload(np.full(n, 7, np.uint32))
    in_d, ch_d = hipmem.DeviceBuffer(6 * 8).upload(np.full(6, 7, np.uint64)), hipmem.DeviceBuffer(5 * 4).upload(np.full(5, 7, np.uint32))
    J.seed_histogram_centroids_d(n, 10, hist_d.ptr, 8, cen_d.ptr, seed=SEED, nonce=3, stream=stream)
    J.cluster_histograms_d(n, 10, hist_d.ptr, 8, cen_d.ptr, 5, label_d.ptr, dist_d.ptr, in_d.ptr, ch_d.ptr, stream=stream)
    assert hip.hipStreamSynchronize(stream) == 0
    assert np.array_equal(cen_d.download(np.uint16, 80).reshape(8, 10), want["centroids"])
    assert np.array_equal(label_d.download(np.uint16, n), want["labels"]) and np.array_equal(dist_d.download(np.uint32, n), want["dist"])
    assert np.array_equal(in_d.download(np.uint64, 6), want["inertia"]) and np.array_equal(ch_d.download(np.uint32, 5), want["changed"])
    label_d.upload(np.full(n, 7, np.uint16))
    J.assign_histograms_d(n, 10, hist_d.ptr, 8, cen_d.ptr, label_d.ptr, None, stream=stream)   # dist not wanted
    assert hip.hipStreamSynchronize(stream) == 0
    assert np.array_equal(label_d.download(np.uint16, n), want["labels"])
    assert hip.hipStreamDestroy(stream) == 0
    for x in (hist_d, cen_d, label_d, dist_d, in_d, ch_d):
        x.free()


def test_one_board_and_one_histogram_against_4096_centroids(PK):
    from pokerl_amd import judger as J
    train = rows(41, 6000, 10)
    cen = centroids_near(42, train, 4096)
    board = rows(43, 1326, 10, empty_frac=0.15)                      # one board's holdings against PK_CL_MAX_K buckets
    label, _ = check_assign(J, board, cen)
    assert len(set(label.tolist())) > 100
    r = J.HistogramClusters(cen, None, None, np.zeros(1, np.uint64), np.zeros(0, np.uint32))
    one_label, one_dist = r.assign(board[board.any(axis=1)][:1])     # a single histogram
    q, empty = CS.quant(board[board.any(axis=1)][:1])
    want_l, want_d = CS.assign(q, empty, cen)
    assert one_label.shape == (1,) and np.array_equal(one_label, want_l) and np.array_equal(one_dist, want_d)


def test_argument_errors_leave_the_outputs_untouched(PK):
    from pokerl_amd import _lib as L
    lib = L.lib()
    hist = rows(3, 40, 4, empty_frac=0.0)
    cen, label, dist = np.full((2, 4), 7, np.uint16), np.full(40, 7, np.uint16), np.full(40, 7, np.uint32)
    inertia, changed = np.full(3, 7, np.uint64), np.full(2, 7, np.uint32)
    p = L.ptr
    bad = L.PK_E_INVALID_ARG
    assert lib.pk_hist_cluster_seed(0, 40, 33, p(hist), 2, 1, 0, p(cen)) == bad
    assert lib.pk_hist_cluster_seed(0, 40, 4, p(hist), 4097, 1, 0, p(cen)) == bad
    assert lib.pk_hist_cluster_seed(0, 40, 4, p(hist), 41, 1, 0, p(cen)) == bad
    assert lib.pk_hist_cluster_assign(0, 0, 4, p(hist), 2, p(cen), p(label), p(dist)) == bad
    assert lib.pk_hist_cluster_assign(0, 40, 4, p(hist), 4097, p(cen), p(label), p(dist)) == bad
    assert lib.pk_hist_cluster(0, 1, 4, p(hist), 2, p(cen), 2, p(label), p(dist), p(inertia), p(changed)) == bad   # K > n: clustering, not assign
    assert lib.pk_hist_cluster(0, 40, 4, p(hist), 2, p(cen), 0, p(label), p(dist), p(inertia), p(changed)) == bad
    assert lib.pk_hist_cluster(0, 40, 4, p(hist), 2, p(cen), 1025, p(label), p(dist), p(inertia), p(changed)) == bad
    assert lib.pk_hist_cluster(0, 40, 0, p(hist), 2, p(cen), 2, p(label), p(dist), p(inertia), p(changed)) == bad
    few = hist.copy()
    few[1:] = 0                                                      # one non-empty row, K = 2
    assert lib.pk_hist_cluster(0, 40, 4, p(few), 2, p(cen), 2, p(label), p(dist), p(inertia), p(changed)) == bad
    assert lib.pk_hist_cluster_seed(0, 40, 4, p(np.zeros_like(hist)), 1, 1, 0, p(cen)) == bad
    assert lib.pk_hist_cluster_seed_d(0, 40, 4, None, 2, 1, 0, None, None) == bad
    assert lib.pk_hist_cluster_d(0, 2 ** 31, 4, 1, 2, 1, 2, 1, None, None, None, None) == bad
    assert lib.pk_hist_cluster_assign_d(64, 40, 4, 1, 2, 1, 1, None, None) != L.PK_OK   # no such device
    for a in (cen, label, dist, inertia, changed):
        assert (a == 7).all()
