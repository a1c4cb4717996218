"""Identity clustering on the device (next-row f6): from the face embeddings of a ragged batch of videos to each face's identity
index, and from there to the `sequence.Identity` lists `sequence.plan_clip` takes.

The reference does this on the host, once per video: `similarities = np.dot(E, E.T)` on FaceNet embeddings copied back from the
device, then `_generate_connected_components` (preprocessing/utils.py:16-29; called at preprocessing/cluster_faces.py:96-101 and
predict.py:162-167 with threshold 0.45), a Python double loop over all n^2 entries feeding a networkx graph.  Here it is one short
chain of launches with no host read (csrc/identity.hip; the rule is stated in include/mintime_hip.h):

  * i -- j iff i != j and s_ij > threshold (strict; NaN is no edge), s = the fp32 dot product, never across videos;
  * a face without an edge is labelled -1: the reference never adds it to the graph, it stays a loose file (the dataset's
    `discarded_faces`);
  * every other face gets the 0-based rank of its connected component among its video's components ordered by smallest member,
    the order in which `nx.connected_components` yields them for the graph that function builds from a symmetric matrix.  From an
    asymmetric matrix (`cluster_similarities` only) the reference lists a component at the first row that holds one of its entries
    above the threshold, which need not be its smallest member; the kernels rank by that row there, so the order still matches.

Thresholds are compared in fp32, like the similarities.  Not covered: the embedding network, `valid_cluster_size` (the reference
computes it and never uses it), moving files."""
from typing import List, Sequence, Tuple

import numpy as np
import torch

from . import lib as L
from .sequence import Identity

MAX_FACES = 4096         # faces of one video: its labels live in LDS (csrc/identity.hip)
MAX_DIM = 2048
TILE = 32                # side of a Gram tile = bits of an adjacency word

ERR_TRUNCATED, ERR_NOT_CONVERGED, ERR_OFFSETS = 1, 2, 4      # bits of the sticky error flag (include/mintime_hip.h)


def _check_counts(counts):
    counts = [int(c) for c in counts]
    if not counts or any(c < 0 for c in counts):
        raise ValueError("counts: one non-negative face count per video, at least one video")
    if max(counts) > MAX_FACES:
        raise NotImplementedError(f"{max(counts)} faces in one video: the clustering kernels hold a video's labels in LDS, "
                                  f"at most {MAX_FACES} faces")
    return counts


def _check_dim(dim):
    if not 1 <= int(dim) <= MAX_DIM:
        raise NotImplementedError(f"embedding width {dim} is outside 1..{MAX_DIM}")
    return int(dim)


def _check_embeddings(embeddings, counts, dim=None):
    if not (torch.is_tensor(embeddings) and embeddings.is_cuda):
        raise ValueError("identity clustering: embeddings must be a tensor on the device (there is no CPU path)")
    if embeddings.dtype != torch.float32 or embeddings.dim() != 2:
        raise ValueError(f"identity clustering: embeddings must be fp32 [faces, dim], got {embeddings.dtype} {tuple(embeddings.shape)}")
    if sum(counts) != embeddings.shape[0]:
        raise ValueError(f"identity clustering: counts add up to {sum(counts)} faces, embeddings hold {embeddings.shape[0]}")
    if dim is not None and embeddings.shape[1] != dim:
        raise ValueError(f"identity clustering: the plan was built for dim = {dim}, embeddings have {embeddings.shape[1]}")


def _raise_on_flag(flag):
    if flag:
        what = [text for bit, text in ((ERR_TRUNCATED, "a video holds more faces than the plan's max_faces (treated as truncated)"),
                                       (ERR_NOT_CONVERGED, "the label loop hit its trip bound (the adjacency was not symmetric)"),
                                       (ERR_OFFSETS, "video offsets outside the embedding rows")) if flag & bit]
        raise L.MintimeHipError(f"identity clustering set its error flag to {flag}: " + "; ".join(what))


def identities_from_labels(labels, offsets, faces):
    """Pure host grouping.  labels: [T] identity index per face (-1 = no identity); offsets: V + 1 row offsets; faces: per video, the
    (frame, height, width) tuple of every face in row order.  -> per video (List[Identity], discarded): identities named "0", "1", ...
    (the folder names of cluster_faces.py:109) with their members in index order, and the indices labelled -1."""
    labels = [int(x) for x in np.asarray(labels).reshape(-1)]
    if len(faces) != len(offsets) - 1:
        raise ValueError(f"faces lists {len(faces)} videos, offsets describe {len(offsets) - 1}")
    out = []
    for v, video_faces in enumerate(faces):
        lab = labels[offsets[v]:offsets[v + 1]]
        if len(video_faces) != len(lab):
            raise ValueError(f"video {v}: {len(video_faces)} faces given, {len(lab)} rows clustered")
        members = [[] for _ in range(max(lab, default=-1) + 1)]
        discarded = []
        for i, (k, face) in enumerate(zip(lab, video_faces)):
            if k < 0:
                discarded.append(i)
            else:
                members[k].append(tuple(face))
        out.append(([Identity(str(k), m) for k, m in enumerate(members)], discarded))
    return out


class IdentityClusters:
    """labels [T], n_identities [V], sizes [T] (sizes[offsets[v] + k] = members of identity k of video v, 0 beyond n_identities[v]):
    int32 device tensors; offsets: host list of V + 1 row offsets.  The tensors belong to the plan that produced them and are
    overwritten by its next run."""

    def __init__(self, labels, n_identities, sizes, offsets, err_flag):
        self.labels, self.n_identities, self.sizes, self.offsets = labels, n_identities, sizes, list(offsets)
        self._err = err_flag

    def host_labels(self):
        """The labels as a numpy array; synchronises, and reports a set error flag."""
        flag = int(self._err.cpu()[0])          # (a synchronising copy on the current stream: the labels are complete after it)
        _raise_on_flag(flag)
        return self.labels.cpu().numpy()

    def components(self):
        """Per video, the list of sorted member lists, in identity order: for one video exactly
        [sorted(c) for c in _generate_connected_components(similarities, threshold)].  Synchronises."""
        lab = self.host_labels()
        out = []
        for v in range(len(self.offsets) - 1):
            l = lab[self.offsets[v]:self.offsets[v + 1]]
            comps = [[] for _ in range(int(l.max()) + 1 if l.size else 0)]
            for i, k in enumerate(l.tolist()):
                if k >= 0:
                    comps[k].append(i)
            out.append(comps)
        return out

    def identities(self, faces):
        """faces: per video, the (frame, height, width) tuples in row order -> per video (List[sequence.Identity], discarded), ready
        for sequence.plan_clip.  Synchronises."""
        return identities_from_labels(self.host_labels(), self.offsets, faces)


class ClusterPlan:
    """The clustering of one batch shape: `counts` faces per video (host ints), embeddings of width `dim`.

        plan = ClusterPlan([len(f) for f in faces_per_video], 512)
        clusters = plan.run(embeddings)                 # two launches on the current stream, nothing read back
        for ids, discarded in clusters.identities(faces_per_video): ...

    The constructor uploads the row offsets and the tile prefix once and owns the adjacency and the outputs; `run` only launches, so
    it can sit inside a captured graph.  `adjacency` is the [T, W] bit matrix, W = ceil(max_faces / 32) int32 words a row."""

    def __init__(self, counts: Sequence[int], dim: int, device="cuda"):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise ValueError("ClusterPlan lives on the device (there is no CPU path)")
        self.counts = _check_counts(counts)
        self.dim = _check_dim(dim)
        self.device = dev
        V, T = len(self.counts), sum(self.counts)
        self.max_faces = max(1, max(self.counts))
        self.words = (self.max_faces + TILE - 1) // TILE
        self.offsets = [0] * (V + 1)
        prefix = [0] * (V + 1)
        for v, c in enumerate(self.counts):
            self.offsets[v + 1] = self.offsets[v] + c
            prefix[v + 1] = prefix[v] + ((c + TILE - 1) // TILE) ** 2
        if prefix[-1] >= 1 << 31:
            raise NotImplementedError(f"{prefix[-1]} Gram tiles in one batch: the grid is a 32-bit count")
        self.total_tiles = prefix[-1]
        packed = torch.tensor(self.offsets + prefix, dtype=torch.int32).pin_memory()
        self._index = packed.to(dev, non_blocking=True)
        self._offsets_dev, self._prefix_dev = self._index[:V + 1], self._index[V + 1:]
        self.adjacency = torch.empty(max(T, 1), self.words, dtype=torch.int32, device=dev)[:T]
        self.labels = torch.empty(max(T, 1), dtype=torch.int32, device=dev)[:T]
        self.sizes = torch.empty(max(T, 1), dtype=torch.int32, device=dev)[:T]
        self.n_identities = torch.empty(V, dtype=torch.int32, device=dev)
        self.err_flag = L.zeros(1, torch.int32, dev)

    @torch.no_grad()
    def run(self, embeddings, similarity_threshold=0.45):
        """embeddings [T, dim] fp32 on the device, rows in video order -> IdentityClusters (views of this plan's buffers)."""
        _check_embeddings(embeddings, self.counts, self.dim)
        e = embeddings.detach().contiguous()
        V, T = len(self.counts), sum(self.counts)
        L.mt.identity_adjacency(e, self._offsets_dev, self._prefix_dev, V, T, self.dim, self.total_tiles, self.max_faces,
                                float(similarity_threshold), self.adjacency, self.err_flag)
        L.mt.identity_components(self.adjacency, self._offsets_dev, None, V, T, self.max_faces, self.labels, self.n_identities, self.sizes,
                                 self.err_flag)
        return IdentityClusters(self.labels, self.n_identities, self.sizes, self.offsets, self.err_flag)


def cluster_embeddings(embeddings, counts, similarity_threshold=0.45):
    """Build a ClusterPlan for `counts` faces per video and run it once.  0.45 is the threshold both reference call sites pass."""
    counts = _check_counts(counts)
    _check_embeddings(embeddings, counts)
    return ClusterPlan(counts, embeddings.shape[1], embeddings.device).run(embeddings, similarity_threshold)


@torch.no_grad()
def cluster_similarities(similarities, similarity_threshold=0.80):
    """One video from a ready similarity matrix [n, n] fp32 (need not be symmetric): the reference function's own signature and
    default threshold.  An edge is either order above the threshold, as the reference visits both."""
    s = similarities
    if not (torch.is_tensor(s) and s.is_cuda):
        raise ValueError("cluster_similarities: similarities must be a tensor on the device (there is no CPU path)")
    if s.dtype != torch.float32 or s.dim() != 2 or s.shape[0] != s.shape[1]:
        raise ValueError(f"cluster_similarities: similarities must be a square fp32 matrix, got {s.dtype} {tuple(s.shape)}")
    n = _check_counts([s.shape[0]])[0]
    s = s.detach().contiguous()
    dev, words = s.device, (max(n, 1) + TILE - 1) // TILE
    offsets = torch.tensor([0, n], dtype=torch.int32).pin_memory().to(dev, non_blocking=True)
    adj = torch.empty(max(n, 1), words, dtype=torch.int32, device=dev)[:n]
    labels = torch.empty(max(n, 1), dtype=torch.int32, device=dev)[:n]
    sizes = torch.empty(max(n, 1), dtype=torch.int32, device=dev)[:n]
    source = torch.empty(max(n, 1), dtype=torch.int32, device=dev)[:n]
    n_identities = torch.empty(1, dtype=torch.int32, device=dev)
    err = L.zeros(1, torch.int32, dev)
    L.mt.identity_adjacency_sim(s, n, float(similarity_threshold), adj, source)
    L.mt.identity_components(adj, offsets, source, 1, n, max(n, 1), labels, n_identities, sizes, err)
    out = IdentityClusters(labels, n_identities, sizes, [0, n], err)
    out.adjacency = adj
    return out
