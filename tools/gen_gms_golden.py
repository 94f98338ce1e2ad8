"""Records tests/golden/gms_*.npz from the reference's own clustering functions.

    python3 tools/gen_gms_golden.py /path/to/reference [--out tests/golden]

Reads the reference AT GENERATION TIME: uois/src/cluster.py is executed as it stands, as a module of a stand-in package whose ``.util``
is an empty module (it imports one and never uses it); ``DSNWrapper.cluster`` is pulled out of uois/src/segmentation.py by `ast` and run
unmodified on CPU tensors with a stand-in config, ``OBJECTS_LABEL = 2`` and the executed cluster module.  Nothing of the reference is
in this file, and the fixtures are data.  Per scene (tests/test_gms_cpu.py: vote_scene):
  (a) with a subclass of the reference's GaussianMeanShift whose select_smart_seeds returns the CONTRACT's seeds (seeds_np): the
      selected indices, the reference's climbed seeds, seed labels, the clustered image of its cluster() and uniq_cluster_centers;
  (b) with the reference's own multinomial seeding: the clustered image only.
The reference numbers its objects from OBJECTS_LABEL = 2; the fixtures store 1..count.  gms_link_chains.npz: hand-built seed sets
(chain_cases) with the labels the reference's connected_components gives them."""
import argparse
import ast
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

CONFIG = dict(max_GMS_iters=10, epsilon=0.05, sigma=0.02, num_seeds=40, subsample_factor=5, min_pixels_thresh=20)


def load_cluster_module(path):
    """uois/src/cluster.py as a module of a stand-in package with an empty `.util.utilities`."""
    pkg = types.ModuleType("gms_ref_pkg")
    pkg.__path__ = []
    util = types.ModuleType("gms_ref_pkg.util")
    util.__path__ = []
    util.utilities = types.ModuleType("gms_ref_pkg.util.utilities")
    sys.modules.update({"gms_ref_pkg": pkg, "gms_ref_pkg.util": util, "gms_ref_pkg.util.utilities": util.utilities})
    mod = types.ModuleType("gms_ref_pkg.cluster")
    mod.__package__ = "gms_ref_pkg"
    exec(compile(open(path).read(), path, "exec"), mod.__dict__)
    return mod


def load_cluster_method(path, cluster_ns):
    """DSNWrapper.cluster on a holder object with a stand-in config."""
    tree = ast.parse(open(path).read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "DSNWrapper")
    fn = next(f for f in cls.body if isinstance(f, ast.FunctionDef) and f.name == "cluster")
    holder = ast.ClassDef(name="Holder", bases=[], keywords=[], body=[fn], decorator_list=[])
    if "type_params" in ast.ClassDef._fields:
        holder.type_params = []
    env = {"torch": torch, "np": np, "cluster": cluster_ns, "OBJECTS_LABEL": 2}
    exec(compile(ast.fix_missing_locations(ast.Module([holder], [])), path, "exec"), env)
    obj = env["Holder"]()
    obj.config, obj.device = dict(CONFIG), "cpu"
    return obj


def from_two(img):
    """The reference's 0, 2, 3, ... -> 0, 1, 2, ..."""
    a = img.numpy().astype(np.int32)
    return np.where(a > 0, a - 1, 0).astype(np.int32)


def record(ref, seg_path, votes, fg, seed):
    from test_gms_cpu import compact_np, seeds_np
    from quber_amd.gms import GaussianMeanShift
    sub, S = CONFIG["subsample_factor"], CONFIG["num_seeds"]
    _, Xs = compact_np(votes, fg, sub)
    assert len(Xs) >= S, "the reference leaves seeds uninitialised when there are fewer points than seeds"
    first, draws = GaussianMeanShift(num_seeds=S, seed=seed).draws([len(Xs)])
    idx = seeds_np(Xs, first[0], draws[0], S)
    kept = {}

    class ContractSeeds(ref.GaussianMeanShift):
        def select_smart_seeds(self, X):
            assert np.array_equal(X.numpy(), Xs)
            return X[torch.from_numpy(idx.astype(np.int64))].clone()

        def mean_shift_with_seeds(self, X, Z):
            labels, Zc = super().mean_shift_with_seeds(X, Z)
            kept["seed_labels"], kept["seeds"] = labels.numpy().astype(np.int32), Zc.numpy().astype(np.float32)
            return labels, Zc

    t_votes, t_fg = torch.from_numpy(votes), torch.from_numpy(fg.astype(bool))
    ns = types.SimpleNamespace(GaussianMeanShift=ContractSeeds)
    img, centers = load_cluster_method(seg_path, ns).cluster(t_votes, torch.zeros_like(t_votes), t_fg)
    np.random.seed(seed)
    torch.manual_seed(seed)
    img_b, _ = load_cluster_method(seg_path, ref).cluster(t_votes, torch.zeros_like(t_votes), t_fg)
    return dict(votes=votes, fg=fg, first=np.int32(first[0]), draws=draws[0], indices=idx, seeds=kept["seeds"], seed_labels=kept["seed_labels"],
                clustered=from_two(img), centers=centers.numpy().astype(np.float32), clustered_multinomial=from_two(img_b),
                num_seeds=np.int32(S), sigma=np.float32(CONFIG["sigma"]), iters=np.int32(CONFIG["max_GMS_iters"]),
                epsilon=np.float32(CONFIG["epsilon"]), subsample=np.int32(sub), min_pixels=np.int32(CONFIG["min_pixels_thresh"]))


def main():
    from test_gms_cpu import chain_cases, vote_scene
    ap = argparse.ArgumentParser()
    ap.add_argument("reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    ref = load_cluster_module(os.path.join(a.reference, "uois", "src", "cluster.py"))
    seg_path = os.path.join(a.reference, "uois", "src", "segmentation.py")
    chains = {}
    ms = ref.GaussianMeanShift(epsilon=0.05)
    for name, (Z, _) in chain_cases().items():
        chains[name + "_seeds"] = Z
        chains[name + "_labels"] = ms.connected_components(torch.from_numpy(Z)).numpy().astype(np.int32)
    path = os.path.join(a.out, "gms_link_chains.npz")
    np.savez_compressed(path, **chains)
    print(path, os.path.getsize(path), "bytes;", {k: v.tolist() for k, v in chains.items() if k.endswith("_labels")})
    for (h, w), k, s in (((24, 32), 3, 11), ((37, 53), 4, 12)):
        votes, fg, _ = vote_scene(h, w, k, s, stray=3)
        r = record(ref, seg_path, votes, fg, s)
        path = os.path.join(a.out, f"gms_scene_{h}x{w}.npz")
        np.savez_compressed(path, **r)
        print(path, os.path.getsize(path), "bytes;", r["clustered"].max(), "clusters with the contract's seeds,", r["clustered_multinomial"].max(),
              "with the reference's; seed labels", len(np.unique(r["seed_labels"])))


if __name__ == "__main__":
    main()
