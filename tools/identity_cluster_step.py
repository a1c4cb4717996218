#!/usr/bin/env python3
"""What the identity clustering costs on the device: `ClusterPlan.run` (mt_identity_adjacency + mt_identity_components, csrc/identity.hip)
timed with device events, warm, as the median (with min and max) of `--rounds` windows of `--calls` back-to-back calls, at

  (a) batch   V = 64 videos of 200 faces, D = 512 (three identities and a few loose faces per video)
  (b) single  one video of 800 faces, D = 512, one large component

plus each of the two launches alone at the same shapes, and the same `run` replayed from a captured graph.  The same process then times
the numpy restatement the tests use (tests/identity_ref.py: an fp32 Gram matrix per video, a vectorised comparison, union-find in
Python) on this host, one run per shape, and checks that both give the same labels.  Prints one JSON line.

    python tools/identity_cluster_step.py --rounds 7 --calls 200
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import mintime_amd  # noqa: E402,F401
from mintime_amd import ClusterPlan, lib  # noqa: E402
from tests import identity_ref  # noqa: E402

THRESHOLD = 0.45


def median(v):
    s = sorted(v)
    return s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])


def events(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls          # microseconds per call


def windows(fn, rounds, calls):
    events(fn, max(10, calls // 10))                  # warm: code objects loaded, clocks up
    v = [events(fn, calls) for _ in range(rounds)]
    return {"median_us": round(median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)}


def video(rng, n, dim, identities, loose, spread=0.8):
    """Unit vectors around `identities` random centres (similarity within an identity about 1 / (1 + spread^2) = 0.61, across about 0
    +- 1 / sqrt(dim)) and `loose` faces that belong to none."""
    centres = rng.standard_normal((identities, dim))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    which = rng.integers(0, identities, n)
    e = centres[which] + spread * rng.standard_normal((n, dim)) / np.sqrt(dim)
    e[rng.choice(n, loose, replace=False)] = rng.standard_normal((loose, dim))
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    return e.astype(np.float32)


def measure(name, emb, counts, a):
    dim = emb.shape[1]
    dev = torch.from_numpy(emb).cuda()
    plan = ClusterPlan(counts, dim)
    out = {"shape": f"V={len(counts)} x {max(counts)} faces, D={dim}", "tiles": plan.total_tiles, "words_per_row": plan.words}
    out["run"] = windows(lambda: plan.run(dev, THRESHOLD), a.rounds, a.calls)
    L, V, T, st = lib.get(), len(counts), sum(counts), lib.stream_ptr()
    out["adjacency_alone"] = windows(lambda: lib.check(L.mt_identity_adjacency(
        lib.ptr(dev), lib.ptr(plan._offsets_dev), lib.ptr(plan._prefix_dev), V, T, dim, plan.total_tiles, plan.max_faces, THRESHOLD,
        lib.ptr(plan.adjacency), lib.ptr(plan.err_flag), st), "mt_identity_adjacency"), a.rounds, a.calls)
    out["components_alone"] = windows(lambda: lib.check(L.mt_identity_components(
        lib.ptr(plan.adjacency), lib.ptr(plan._offsets_dev), None, V, T, plan.max_faces, lib.ptr(plan.labels), lib.ptr(plan.n_identities),
        lib.ptr(plan.sizes), lib.ptr(plan.err_flag), st), "mt_identity_components"), a.rounds, a.calls)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = plan.run(dev, THRESHOLD)
    out["graph_replay"] = windows(graph.replay, a.rounds, a.calls)
    labels = got.host_labels()
    n_ids = got.n_identities.cpu().numpy()
    t0 = time.perf_counter()
    want_labels, want_n, _ = identity_ref.cluster_embeddings(emb, counts, THRESHOLD, np.float32)
    out["numpy_restatement_host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    out["min_margin_fp64"] = float(f"{identity_ref.min_margin(emb, counts, THRESHOLD):.3g}")
    out["labels_equal_restatement"] = bool(np.array_equal(labels, want_labels) and np.array_equal(n_ids, want_n))
    out["identities_per_video"] = [int(n_ids.min()), int(n_ids.max())]
    out["faces_without_identity"] = int((labels < 0).sum())
    out["flops_gram"] = 2 * plan.total_tiles * 32 * 32 * dim
    return name, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("identity_cluster_step.py needs a GPU")
    lib.get()
    rng = np.random.default_rng(0)
    batch = np.concatenate([video(rng, 200, 512, 3, 6) for _ in range(64)])
    single = video(rng, 800, 512, 1, 0)
    out = {"threshold": THRESHOLD, "rounds": a.rounds, "calls_per_window": a.calls}
    for name, res in (measure("batch", batch, [200] * 64, a), measure("single", single, [800], a)):
        out[name] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
