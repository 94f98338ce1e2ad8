"""Records tests/golden/meanshift_*.npz from the reference's own clustering functions.

    python3 tools/gen_meanshift_golden.py /path/to/reference [--out tests/golden]

Reads eval/base_model.py of the reference AT GENERATION TIME, pulls the eight methods of the UCN base model's clustering
(clustering_features, mean_shift_smart_init, select_smart_seeds, connected_components, seed_hill_climbing_ball, mean_shift_with_seeds,
ball_kernel, get_label_mode) and the module-level filter_labels_depth out of it by `ast`, and runs them unmodified on CPU tensors with a
stand-in `cfg` (TRAIN.EMBEDDING_METRIC = "cosine", TRAIN.EMBEDDING_ALPHA = 0.02).  Nothing of the reference is in this file, and the
fixtures are data: inputs (float16: every value is float16-representable), selected indices, climbed seeds, seed labels, label maps, the
depth plane and the filtered map; and meanshift_link_chains.npz: hand-built seed sets (chain_cases) with the labels the reference's
connected_components gives them.  The inputs come from tests/test_meanshift_cpu.py (blob_embeddings, grid_embeddings)."""
import argparse
import ast
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

METHODS = ("clustering_features", "mean_shift_smart_init", "select_smart_seeds", "connected_components", "seed_hill_climbing_ball",
           "mean_shift_with_seeds", "ball_kernel", "get_label_mode")


def load_reference(path):
    """-> (an object with the eight methods bound and a stand-in cfg, filter_labels_depth)."""
    src = open(path).read()
    tree = ast.parse(src)
    env = {"torch": torch, "np": np, "F": F}
    flt = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "filter_labels_depth")
    exec(compile(ast.Module([flt], []), path, "exec"), env)
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef)
               and set(METHODS) <= {f.name for f in n.body if isinstance(f, ast.FunctionDef)})
    picked = [f for f in cls.body if isinstance(f, ast.FunctionDef) and f.name in METHODS]
    holder = ast.ClassDef(name="Clustering", bases=[], keywords=[], body=picked, decorator_list=[])
    if "type_params" in ast.ClassDef._fields:
        holder.type_params = []
    exec(compile(ast.fix_missing_locations(ast.Module([holder], [])), path, "exec"), env)
    obj = env["Clustering"]()
    obj.cfg = types.SimpleNamespace(TRAIN=types.SimpleNamespace(EMBEDDING_METRIC="cosine", EMBEDDING_ALPHA=0.02))
    return obj, env["filter_labels_depth"]


def record(obj, flt, emb, which, num_seeds, seed, threshold, drop):
    h, w = emb.shape[1:]
    feats = torch.from_numpy(emb)[None]
    # clustering_features discards the climbed seeds and the seed labels: run its steps as it does and keep them
    np.random.seed(seed)
    X = feats[0].view(feats.shape[1], -1).t()
    seeds, sel = obj.select_smart_seeds(X, num_seeds, return_selected_indices=True, metric="cosine")
    seed_labels, Z = obj.mean_shift_with_seeds(X, seeds, 20, max_iters=10, metric="cosine")
    np.random.seed(seed)
    labels, sel2 = obj.clustering_features(feats, num_seeds=num_seeds)
    assert torch.equal(sel, sel2[0])
    # a depth plane that starves cluster `drop` of depth: positive z on a quarter of its pixels, everywhere else on all
    rng = np.random.RandomState(seed)
    z = np.ones((h, w), np.float32)
    z[(which == drop) & (rng.rand(h, w) < 0.75)] = 0
    depth = torch.zeros((1, 3, h, w))
    depth[0, 2] = torch.from_numpy(z)
    filtered = flt(labels, depth, threshold)[0].numpy()
    out = np.zeros((h, w), np.int32)
    for k, l in enumerate(u for u in np.unique(filtered) if u != 0):       # predict()'s np.unique loop: survivors numbered 1..count
        out[filtered == l] = k + 1
    return dict(emb=emb.astype(np.float16), indices=sel.numpy().astype(np.int32), seeds=Z.numpy().astype(np.float32),
                seed_labels=seed_labels.numpy().astype(np.int32), labels=labels[0].numpy().astype(np.int32), depth_z=z,
                filtered=out, threshold=np.float32(threshold), num_seeds=np.int32(num_seeds), kappa=np.float32(20), iters=np.int32(10),
                epsilon=np.float32(0.04))


def main():
    from test_meanshift_cpu import blob_embeddings, chain_cases, grid_embeddings
    ap = argparse.ArgumentParser()
    ap.add_argument("reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    obj, flt = load_reference(os.path.join(a.reference, "eval", "base_model.py"))
    # the hand-built seed sets with non-transitive balls, through the reference's connected_components: the mode branch
    chains = {}
    for name, (Z, _) in chain_cases().items():
        chains[name + "_seeds"] = Z
        chains[name + "_labels"] = obj.connected_components(torch.from_numpy(Z), 0.04, metric="cosine").numpy().astype(np.int32)
    path = os.path.join(a.out, "meanshift_link_chains.npz")
    np.savez_compressed(path, **chains)
    print(path, os.path.getsize(path), "bytes;", {k: v.tolist() for k, v in chains.items() if k.endswith("_labels")})
    for kind, make in (("blob", blob_embeddings), ("grid", grid_embeddings)):
        for (h, w), k, s, seeds in (((24, 32), 4, 11, 100), ((37, 53), 5, 12, 33)):
            emb, which = make(h, w, k, s)
            assert np.array_equal(emb.astype(np.float16).astype(np.float32), emb)
            r = record(obj, flt, emb, which, seeds, s, 0.5, drop=1)
            path = os.path.join(a.out, f"meanshift_{kind}_{h}x{w}.npz")
            np.savez_compressed(path, **r)
            print(path, os.path.getsize(path), "bytes;", len(np.unique(r["labels"])), "clusters,", r["filtered"].max(), "after the depth filter")


if __name__ == "__main__":
    main()
