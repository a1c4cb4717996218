"""numpy restatement of the identity-clustering rule (include/mintime_hip.h, "Identity clustering"): what the GPU tests compare
against on a machine that has neither the reference nor networkx.  tests/test_identity_host.py holds it to the outputs of the
reference's _generate_connected_components recorded in tests/golden/identity_components.json, order included.

  edge    i -- j iff i != j and s_ij > threshold (strict, fp32 comparison; NaN is no edge); from a similarity matrix either order counts
  label   -1 for a face without an edge, otherwise the 0-based rank of its component among the components ordered by their smallest
          SOURCE: a member whose own row holds an entry above the threshold.  networkx lists components in node-insertion order and
          the reference's loop inserts a component's first node at that row.  For a symmetric matrix (every Gram matrix) every face
          with an edge is a source, so the order is by smallest member.
"""
import numpy as np


def edges_from_similarities(sim, threshold):
    """([n, n] bool edges, [n] bool sources): the reference visits (i, j) and (j, i) and its graph is undirected."""
    s = np.asarray(sim, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        above = s > np.float32(threshold)
    above = above.copy()
    np.fill_diagonal(above, False)
    return above | above.T, above.any(axis=1)


def edges_from_gram(gram, threshold):
    """[n, n] bool from a Gram matrix of any precision: i != j and g_ij > threshold (the threshold rounded to fp32, as the kernels
    take it)."""
    g = np.asarray(gram)
    with np.errstate(invalid="ignore"):
        e = g > g.dtype.type(np.float32(threshold))
    e = e | e.T                  # (a BLAS Gram matrix need not be symmetric to the last bit; the kernels' is)
    np.fill_diagonal(e, False)
    return e


def labels_from_edges(edges, sources=None):
    """(labels [n] int32, n_identities, sizes [n] int32) by union-find whose root is always the smallest member; sources [n] bool
    (default: every face with an edge) decide the order of the components."""
    e = np.asarray(edges, dtype=bool)
    n = e.shape[0]
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for i, j in zip(*np.nonzero(e)):
        a, b = find(int(i)), find(int(j))
        if a != b:
            parent[max(a, b)] = min(a, b)
    has_edge = e.any(axis=1) | e.any(axis=0)
    sources = has_edge if sources is None else np.asarray(sources, dtype=bool) & has_edge
    first = {}
    for i in range(n):
        if sources[i]:
            first.setdefault(find(i), i)
    roots = sorted(first, key=first.get)
    rank = {r: k for k, r in enumerate(roots)}
    labels = np.full(n, -1, np.int32)
    sizes = np.zeros(n, np.int32)
    for i in range(n):
        if has_edge[i]:
            labels[i] = rank[find(i)]
            sizes[labels[i]] += 1
    return labels, len(roots), sizes


def components_from_labels(labels):
    """The sorted member lists in identity order: [sorted(c) for c in _generate_connected_components(...)]."""
    labels = np.asarray(labels)
    out = [[] for _ in range(int(labels.max()) + 1 if labels.size else 0)]
    for i, k in enumerate(labels.tolist()):
        if k >= 0:
            out[k].append(i)
    return out


def cluster_similarities(sim, threshold=0.80):
    return labels_from_edges(*edges_from_similarities(sim, threshold))


def cluster_embeddings(emb, counts, threshold=0.45, dtype=np.float64):
    """Ragged batch: (labels [T], n_identities [V], sizes [T]) with the Gram matrix of every video taken in `dtype`."""
    emb = np.asarray(emb)
    labels, n_ids, sizes, o = [], [], [], 0
    for c in counts:
        e = emb[o:o + c].astype(dtype)
        l, k, s = labels_from_edges(edges_from_gram(e @ e.T, threshold))
        labels.append(l)
        n_ids.append(k)
        sizes.append(s)
        o += c
    return (np.concatenate(labels) if labels else np.zeros(0, np.int32), np.asarray(n_ids, np.int32),
            np.concatenate(sizes) if sizes else np.zeros(0, np.int32))


def min_margin(emb, counts, threshold):
    """The smallest |s_ij - threshold| over every off-diagonal pair of every video, in fp64 (inf when there is no pair)."""
    emb, o, best = np.asarray(emb, dtype=np.float64), 0, np.inf
    for c in counts:
        e = emb[o:o + c]
        g = np.abs(e @ e.T - float(np.float32(threshold)))
        g[np.eye(c, dtype=bool)] = np.inf
        if c > 1:
            best = min(best, float(g.min()))
        o += c
    return best


def unpack_adjacency(words):
    """[rows, W] int32 / uint32 words -> [rows, 32 W] bool (bit j & 31 of word j >> 5 = column j)."""
    w = np.ascontiguousarray(np.asarray(words)).view(np.uint32)
    bits = (w[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None, :]) & 1
    return bits.reshape(w.shape[0], -1).astype(bool)
