"""Identity clustering on the device (mintime_amd.identities; csrc/identity.hip) against the reference's recorded outputs
(tests/golden/identity_components.json) and the numpy restatement tests/identity_ref.py.  Labels, identity counts and sizes are
integers: every comparison is for equality.

Similarity path: the kernel sees the same fp32 matrix as the reference / the restatement, so no margin is involved.
Embedding path: compared with the restatement on the fp64 Gram matrix of the same fp32 embeddings.  Every test asserts first that
every off-diagonal fp64 similarity is at least MARGIN = 1e-3 away from the threshold; the worst-case fp32 dot-product error for
unit vectors at D = 512 is D * 2^-24 ~ 3e-5, so 1e-3 is 30 times the bound and the fp32 decisions equal the fp64 ones.  Two
families have that margin by construction:
  levels  face i of cluster c is cos(t_i) u_c + sin(t_i) w_i with all u, w orthonormal (k + n <= D) and cos(t) from
          {0.95, 0.8, 0.6, 0.3}, the whole set turned by a random orthogonal matrix: similarities are products of two levels within a
          cluster (0.9025 ... 0.09; nearest to 0.45 are 0.48 and 0.36) and 0 across.  Two 0.6-faces are joined only through a brighter
          face; a 0.3-face has no edge and is labelled -1.
  chain   e_i = (u_i + u_{i+1}) / sqrt 2: neighbours 0.5, everything else 0; the graph's diameter is n - 1."""
import json
import os

import numpy as np
import pytest
import torch

from mintime_amd import identities as I
from mintime_amd import lib as L
from mintime_amd import sequence as S
from tests import identity_ref as R
from tests.util import GOLDEN

pytestmark = pytest.mark.gpu

MARGIN = 1e-3
THR = 0.45
LEVELS = (0.95, 0.8, 0.6, 0.3)
SENTINEL = -858993460            # 0xCCCCCCCC


def _cases():
    with open(os.path.join(GOLDEN, "identity_components.json")) as fh:
        rows = json.load(fh)
    for r in rows:
        sim = np.array([[np.nan if x is None else x for x in row] for row in r["similarities"]], dtype=np.float32)
        r["similarities"] = sim.reshape(r["n"], r["n"])
    return rows


CASES = _cases()
_ROT = {}


def _rotation(D):
    """A fixed random orthogonal [D, D] matrix in fp64 (rows orthonormal to ~1e-15)."""
    if D not in _ROT:
        q, r = np.linalg.qr(np.random.default_rng(1000 + D).standard_normal((D, D)))
        _ROT[D] = q * np.sign(np.diag(r))[None, :]
    return _ROT[D]


def levels(n, D, seed, k=3):
    k = min(k, max(1, D - n))
    assert k + n <= D
    rng = np.random.default_rng(seed)
    q = _rotation(D)
    cluster = rng.integers(0, k, n)
    c = np.asarray(LEVELS)[rng.integers(0, len(LEVELS), n)]
    e = c[:, None] * q[cluster] + np.sqrt(1.0 - c * c)[:, None] * q[k + np.arange(n)]
    return e.astype(np.float32)


def chain(n, D, perm_seed=None):
    assert n + 1 <= D
    q = _rotation(D)
    e = (q[:n] + q[1:n + 1]) / np.sqrt(2.0)
    if perm_seed is not None:
        e = e[np.random.default_rng(perm_seed).permutation(n)]
    return e.astype(np.float32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check_embedding_path(emb, counts, thr=THR):
    """Cluster on the device and compare labels, identity counts and sizes with the restatement on the fp64 Gram matrix."""
    assert R.min_margin(emb, counts, thr) >= MARGIN                     # every off-diagonal pair, none excluded
    want_labels, want_n, want_sizes = R.cluster_embeddings(emb, counts, thr, np.float64)
    got = I.cluster_embeddings(_dev(emb), counts, thr)
    labels = got.host_labels()
    assert labels.dtype == np.int32 and got.n_identities.dtype == torch.int32 and got.sizes.dtype == torch.int32
    assert np.array_equal(labels, want_labels)
    assert np.array_equal(got.n_identities.cpu().numpy(), want_n)
    assert np.array_equal(got.sizes.cpu().numpy(), want_sizes)
    return got, want_labels


# ---- similarity path ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_similarity_path_equals_the_recorded_reference_output(case):
    got = I.cluster_similarities(_dev(case["similarities"]), case["threshold"])
    want = case["components"]
    assert got.components() == [want]                                   # order included
    assert got.n_identities.cpu().tolist() == [len(want)]
    assert got.sizes.cpu().tolist() == [len(c) for c in want] + [0] * (case["n"] - len(want))


def test_similarity_path_strictness_and_nan():
    """Entries equal to the threshold and NaN entries are no edge; either order above it is one."""
    nan = np.nan
    s = np.array([[1.0, 0.8125, 0.8125, nan, 0.0, 0.0],
                  [0.8125, 1.0, 0.0, 0.0, 0.0, 0.0],
                  [0.875, 0.0, 1.0, 0.0, 0.0, 0.0],             # (2, 0) above, (0, 2) at the threshold: an edge
                  [nan, 0.0, 0.0, 1.0, nan, 0.0],
                  [0.0, 0.0, 0.0, 0.9, 1.0, 0.0],               # (4, 3) above, (3, 4) NaN: an edge
                  [0.0, 0.0, 0.0, 0.0, 0.0, nan]], dtype=np.float32)
    got = I.cluster_similarities(_dev(s), 0.8125)
    assert got.host_labels().tolist() == [0, -1, 0, 1, 1, -1]
    adj = R.unpack_adjacency(got.adjacency.cpu().numpy())
    assert np.array_equal(adj[:, :6], R.edges_from_similarities(s, 0.8125)[0]) and not adj[:, 6:].any()


@pytest.mark.parametrize("n,symmetric", [(150, False), (150, True), (65, False)])
def test_similarity_path_beyond_one_ballot_and_one_block(n, symmetric):
    """More than 64 columns and more than one block of rows; a sparse asymmetric matrix, where the component order follows the first
    source row (tests/identity_ref.py)."""
    rng = np.random.default_rng(n + symmetric)
    s = (rng.integers(0, 64, (n, n)) / 64.0).astype(np.float32)
    s[rng.random((n, n)) < 1.0 - 1.3 / n] = 0.0                         # about 0.65 entries above the threshold per row
    if symmetric:
        s = np.maximum(s, s.T)
    want_labels, want_n, want_sizes = R.cluster_similarities(s, 0.5)
    assert want_n >= 3 and (want_labels < 0).any()
    got = I.cluster_similarities(_dev(s), 0.5)
    assert np.array_equal(got.host_labels(), want_labels)
    assert got.n_identities.cpu().tolist() == [want_n] and np.array_equal(got.sizes.cpu().numpy(), want_sizes)


def test_similarity_path_empty_video():
    got = I.cluster_similarities(torch.empty(0, 0, device="cuda"))
    assert got.components() == [[]] and got.n_identities.cpu().tolist() == [0]


# ---- embedding path ----------------------------------------------------------------------------------------------------------

LEVEL_SHAPES = [(n, D) for D in (64, 66, 512, 513) for n in (1, 2, 31, 32, 33, 63, 64, 65) if n + 3 <= D]


@pytest.mark.parametrize("n,D", LEVEL_SHAPES)
def test_levels_family(n, D):
    emb = levels(n, D, seed=7 * n + D)
    got, want = _check_embedding_path(emb, [n])
    if n >= 31:
        assert want.max() >= 1 and (want < 0).any()                     # several identities and discarded faces are present


@pytest.mark.parametrize("n,D,perm", [(300, 512, None), (300, 512, 5), (65, 66, None), (65, 66, 6)])
def test_chain_family(n, D, perm):
    """Diameter n - 1; permuted rows make the minimum travel in both directions."""
    got, want = _check_embedding_path(chain(n, D, perm), [n])
    assert (want == 0).all()
    assert got.sizes.cpu().tolist() == [n] + [0] * (n - 1)


@pytest.mark.parametrize("emb,want", [
    ([[1.0], [1.0], [-1.0], [0.5]], [0, 0, -1, 0]),                                                   # D = 1
    ([[1.0, 0.0], [0.0, 1.0], [0.8, 0.6], [0.0, -1.0]], [0, 0, 0, -1]),                               # D = 2
    ([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [0.6, 0.0, 0.8], [0.0, 1.0, 0.0]], [0, 1, 0, 0, 1]),      # D = 3: an odd D
], ids=["D1", "D2", "D3"])
def test_tiny_widths(emb, want):
    emb = np.asarray(emb, dtype=np.float32)
    got, labels = _check_embedding_path(emb, [len(emb)])
    assert labels.tolist() == want


def test_ragged_batch_never_joins_across_videos():
    """Every video is a prefix of the same 64 faces, so a face meets its own copy (similarity 1) in the neighbouring videos."""
    counts = [0, 1, 33, 2, 64, 5]
    base = levels(64, 128, seed=3)
    emb = np.concatenate([base[:c] for c in counts])
    got, labels = _check_embedding_path(emb, counts)
    o = 0
    for v, c in enumerate(counts):
        alone = I.cluster_embeddings(_dev(base[:c]), [c], THR)
        assert np.array_equal(labels[o:o + c], alone.host_labels()), v
        assert int(got.n_identities[v]) == int(alone.n_identities[0])
        o += c
    assert int(got.n_identities[0]) == 0
    comps = got.components()
    assert comps[0] == [] and comps[4] == R.components_from_labels(labels[36:100])


def test_identities_feed_plan_clip():
    n = 33
    emb = levels(n, 64, seed=11)
    faces = [(3 * i, 40 + i % 5, 30 + i % 7) for i in range(n)]
    got = I.cluster_embeddings(_dev(emb), [n], THR)
    (ids, discarded), = got.identities([faces])
    want = R.cluster_embeddings(emb, [n], THR)[0]
    assert discarded == [i for i in range(n) if want[i] < 0] and discarded
    assert [i.name for i in ids] == [str(k) for k in range(int(want.max()) + 1)]
    for k, ident in enumerate(ids):
        assert ident.faces == [faces[i] for i in range(n) if want[i] == k]
    plan = S.plan_clip(ids, num_frames=8, video_wh=(640, 480), max_identities=2, ordering=1)
    assert sum(i.slots for i in plan.identities) == 8


# ---- limits ------------------------------------------------------------------------------------------------------------------

def test_widest_video():
    """4096 identical faces: one identity of 4096 members, W = 128 words a row, every bit but the diagonal set."""
    n = 4096
    emb = np.zeros((n, 8), np.float32)
    emb[:, 2] = 1.0
    plan = I.ClusterPlan([n], 8)
    got = plan.run(_dev(emb), THR)
    assert plan.adjacency.shape == (n, 128)
    assert (got.host_labels() == 0).all()
    assert got.n_identities.cpu().tolist() == [1]
    sizes = got.sizes.cpu().numpy()
    assert sizes[0] == n and not sizes[1:].any()
    adj = R.unpack_adjacency(plan.adjacency.cpu().numpy())
    assert np.array_equal(adj, ~np.eye(n, dtype=bool))


def test_one_face_too_many_is_refused_before_anything_is_written():
    n = 4097
    emb = torch.zeros(n, 8, device="cuda")
    with pytest.raises(NotImplementedError, match="4096"):
        I.cluster_embeddings(emb, [n])
    with pytest.raises(NotImplementedError, match="4096"):
        I.cluster_similarities(torch.zeros(n, n, device="cuda"))
    # the same at the C level, with every output filled with a sentinel beforehand
    lib = L.get()
    words = (n + 31) // 32
    offsets = _dev(np.array([0, n], np.int32))
    prefix = _dev(np.array([0, words * words], np.int32))
    adj = torch.full((n, words), SENTINEL, dtype=torch.int32, device="cuda")
    outs = [torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda") for _ in range(3)] + \
           [torch.full((1,), SENTINEL, dtype=torch.int32, device="cuda") for _ in range(2)]
    labels, sizes, source, n_ids, err = outs
    rc = lib.mt_identity_adjacency(L.ptr(emb), L.ptr(offsets), L.ptr(prefix), 1, n, 8, words * words, n, THR, L.ptr(adj), L.ptr(err),
                                   L.stream_ptr())
    assert rc == -3 and b"4096" in lib.mt_last_error()                  # MT_ERR_UNSUPPORTED
    assert lib.mt_identity_components(L.ptr(adj), L.ptr(offsets), None, 1, n, n, L.ptr(labels), L.ptr(n_ids), L.ptr(sizes), L.ptr(err),
                                      L.stream_ptr()) == -3
    sim = torch.zeros(n, n, device="cuda")
    assert lib.mt_identity_adjacency_sim(L.ptr(sim), n, THR, L.ptr(adj), L.ptr(source), L.stream_ptr()) == -3
    for D in (0, 2049):
        assert lib.mt_identity_adjacency(L.ptr(emb), L.ptr(offsets), L.ptr(prefix), 1, n, D, 1, 4096, THR, L.ptr(adj), L.ptr(err),
                                         L.stream_ptr()) == -3
    assert lib.mt_identity_adjacency(L.ptr(emb), L.ptr(offsets), L.ptr(prefix), 0, n, 8, 1, 4096, THR, L.ptr(adj), L.ptr(err),
                                     L.stream_ptr()) == -1              # V = 0: MT_ERR_ARG
    torch.cuda.synchronize()
    for t in [adj] + outs:
        assert bool((t == SENTINEL).all())
    with pytest.raises(NotImplementedError, match="2048"):
        I.cluster_embeddings(torch.zeros(4, 2049, device="cuda"), [4])


# ---- the adjacency itself ----------------------------------------------------------------------------------------------------

def test_adjacency_is_symmetric_with_zero_diagonal_and_zero_padding():
    """Dense random embeddings, the threshold at the median similarity: about half of the pairs sit on either side and many are
    close to it, so a k order that differed between the triangles would show as an asymmetric bit.  No margin is needed."""
    n, D = 200, 512
    emb = np.random.default_rng(21).standard_normal((n, D)).astype(np.float32)
    emb /= np.linalg.norm(emb, axis=1, keepdims=True)
    g = emb.astype(np.float64) @ emb.astype(np.float64).T
    thr = float(np.float32(np.median(g[~np.eye(n, dtype=bool)])))
    plan = I.ClusterPlan([n], D)
    plan.adjacency.fill_(SENTINEL)
    plan.run(_dev(emb), thr)
    assert plan.adjacency.shape == (n, 7) and plan.adjacency.dtype == torch.int32
    adj = R.unpack_adjacency(plan.adjacency.cpu().numpy())
    assert np.array_equal(adj[:, :n], adj[:, :n].T)
    assert not adj[:, :n].diagonal().any()
    assert not adj[:, n:].any()
    assert 0.4 < adj[:, :n].mean() < 0.6
    clear = np.abs(g - thr) >= MARGIN                                   # where the fp64 value decides beyond fp32's reach: the same bit
    np.fill_diagonal(clear, False)
    assert np.array_equal(adj[:, :n][clear], (g > thr)[clear])


def test_adjacency_rows_and_padding_of_a_ragged_batch():
    """Videos shorter than the widest: their rows are written whole, with zero bits past their own faces."""
    counts = [5, 70, 0, 33]
    base = levels(70, 128, seed=9)
    emb = np.concatenate([base[:c] for c in counts])
    assert R.min_margin(emb, counts, THR) >= MARGIN
    plan = I.ClusterPlan(counts, 128)
    plan.adjacency.fill_(SENTINEL)
    plan.run(_dev(emb), THR)
    adj = R.unpack_adjacency(plan.adjacency.cpu().numpy())
    assert adj.shape == (108, 96)
    o = 0
    for c in counts:
        e = base[:c].astype(np.float64)
        want = np.zeros((c, 96), bool)
        want[:, :c] = R.edges_from_gram(e @ e.T, THR)
        assert np.array_equal(adj[o:o + c], want)
        o += c


# ---- graph capture -----------------------------------------------------------------------------------------------------------

def test_run_replays_from_a_captured_graph():
    """plan.run inside torch.cuda.graph: one linear chain on the capturing stream.  A host read inside run would fail the capture;
    replaying after the embeddings were overwritten in place gives the new labels."""
    n, D = 65, 128
    first, second = levels(n, D, seed=1), chain(n, D, 2)
    counts = [n - 20, 20]
    assert min(R.min_margin(first, counts, THR), R.min_margin(second, counts, THR)) >= MARGIN
    emb = _dev(first)
    plan = I.ClusterPlan(counts, D)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        plan.run(emb, THR)                                              # loads the kernels outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    plan.labels.fill_(SENTINEL)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = plan.run(emb, THR)
    graph.replay()
    assert np.array_equal(got.host_labels(), R.cluster_embeddings(first, counts, THR)[0])
    emb.copy_(_dev(second))
    graph.replay()
    want, want_n, want_sizes = R.cluster_embeddings(second, counts, THR)
    assert np.array_equal(got.host_labels(), want)
    assert np.array_equal(got.n_identities.cpu().numpy(), want_n) and np.array_equal(got.sizes.cpu().numpy(), want_sizes)


# ---- error flag --------------------------------------------------------------------------------------------------------------

def _banded(n, fill=SENTINEL, band=64):
    buf = torch.full((n + 2 * band,), fill, dtype=torch.int32, device="cuda")
    return buf, buf[band:band + n]


def _bands_intact(buf, n, band=64):
    return bool((buf[:band] == SENTINEL).all()) and bool((buf[band + n:] == SENTINEL).all())


def test_understated_max_faces_sets_the_flag_and_stays_in_bounds():
    """A 40-face video under max_faces = 32 (W = 1): it is clustered as its first 32 faces, the rest are labelled -1, bit 0 of the
    flag is set and nothing outside the 40 rows / one word a row is written -- although the tile prefix announces 2 x 2 tiles."""
    n, D, cap = 40, 64, 32
    emb = levels(n, D, seed=13)
    assert R.min_margin(emb[:cap], [cap], THR) >= MARGIN
    lib = L.get()
    e = _dev(emb)
    offsets, prefix = _dev(np.array([0, n], np.int32)), _dev(np.array([0, 4], np.int32))
    adj_buf, adj = _banded(n)                                           # [40][1]
    lab_buf, labels = _banded(n)
    size_buf, sizes = _banded(n)
    nid_buf, n_ids = _banded(1)
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    L.check(lib.mt_identity_adjacency(L.ptr(e), L.ptr(offsets), L.ptr(prefix), 1, n, D, 4, cap, THR, L.ptr(adj), L.ptr(err),
                                      L.stream_ptr()), "mt_identity_adjacency")
    L.check(lib.mt_identity_components(L.ptr(adj), L.ptr(offsets), None, 1, n, cap, L.ptr(labels), L.ptr(n_ids), L.ptr(sizes), L.ptr(err),
                                       L.stream_ptr()), "mt_identity_components")
    torch.cuda.synchronize()
    assert int(err[0]) == I.ERR_TRUNCATED
    assert _bands_intact(adj_buf, n) and _bands_intact(lab_buf, n) and _bands_intact(size_buf, n) and _bands_intact(nid_buf, 1)
    want, want_n, want_sizes = R.cluster_embeddings(emb[:cap], [cap], THR)
    assert labels.cpu().tolist() == want.tolist() + [-1] * (n - cap)
    assert n_ids.cpu().tolist() == want_n.tolist()
    assert sizes.cpu().tolist() == want_sizes.tolist() + [0] * (n - cap)
    a = adj.cpu().numpy()
    assert np.array_equal(R.unpack_adjacency(a[:cap, None])[:, :cap], R.edges_from_gram(emb[:cap].astype(np.float64) @ emb[:cap].astype(np.float64).T, THR))
    assert (a[cap:] == SENTINEL).all()                                  # the rows of the faces past max_faces are not touched
    # the Python surface reports the flag at its synchronising calls
    plan = I.ClusterPlan([n], D)
    plan.max_faces = cap
    got = plan.run(e, THR)
    with pytest.raises(L.MintimeHipError, match="truncated"):
        got.components()
    with pytest.raises(L.MintimeHipError, match="truncated"):
        got.identities([[(0, 1, 1)] * n])
