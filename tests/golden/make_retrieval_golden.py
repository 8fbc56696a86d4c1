"""Golden G10: the database rows the REFERENCE's own retrieval step returns, recorded as data.

    python tests/golden/make_retrieval_golden.py /path/to/reference      # writes tests/golden/g10_retrieval.npz

Run where the reference checkout is; the fixture it writes holds numbers only (descriptors, seeds, flags, returned indices).
Following make_golden.py's habit it runs the reference's own ``SEVEN_SCENES_multi.obtain_KNNs``
(python/niantic/datasets/dataset_7Scenes_multi.py:198-264) on a bare instance (``object.__new__``) with stand-ins for what is
not the rule: stub modules for what the file imports and is not installed (loguru, torchvision, torch_geometric, tqdm, the
vendored sanet loaders, the dataset helpers, path_config), ``SevenSceneManualDataset`` / ``DataLoader`` / ``preprocess_query``
replaced in the module namespace by objects that hand through, ``self.device`` a null context, ``self.vlad_db.forward`` returning
the fixture's query descriptor.  Lines 238-264 -- sklearn's cosine_similarity, np.argsort, the exclusion filters, the two
np.random draws, the strided pick -- run as written.

Three configurations x sampling periods 5 and 10, ``np.random.seed`` fixed per configuration:
  none   test queries against the training split (database_set != query_set: :245-253 not taken)
  self   database_set == query_set: the query, itself a database row, is dropped (:252-253)
  cross  database_set == query_set and cross_connect, scene_seq_len = 10 (:245-250)
Before it writes, the script asserts that tests/retrieval_ref.py + RetrievalRule.reference give exactly the recorded indices.
"""
import contextlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
M, D, G, K, SCENE_SEQ_LEN = 300, 64, 16, 7, 10


class _Pass:
    """Stands for any tensor the loader would hand over: every method the code calls on it returns it."""
    def cuda(self):
        return self

    def clone(self):
        return self

    def squeeze(self, _dim):
        return self


def _stub(name, **attrs):
    mod = types.ModuleType(name)
    mod.__dict__.update(attrs)
    sys.modules[name] = mod
    parent, _, child = name.rpartition(".")
    if parent:
        setattr(sys.modules.get(parent) or _stub(parent), child, mod)
    return mod


def load_reference_module(ref_root):
    anything = type("Anything", (), {"__init__": lambda self, *a, **k: None})
    _stub("loguru", logger=types.SimpleNamespace(info=lambda *a, **k: None))
    _stub("torchvision")
    _stub("torchvision.transforms", Normalize=lambda **k: None)
    _stub("torch_geometric")
    _stub("torch_geometric.data", Data=anything, Dataset=anything, DataLoader=anything)
    if importlib.util.find_spec("tqdm") is None:
        _stub("tqdm", tqdm=lambda it, *a, **k: it)
    for pkg in ("external", "external.sanet_relocal_demo", "external.sanet_relocal_demo.reloc_pipeline",
                "external.sanet_relocal_demo.relocal", "external.sanet_relocal_demo.relocal_data",
                "external.sanet_relocal_demo.relocal_data.seven_scene", "niantic", "niantic.datasets"):
        _stub(pkg)
    _stub("external.sanet_relocal_demo.reloc_pipeline.util_func", preprocess_scene=None, x_2d_coords_torch=None,
          preprocess_query=None)
    _stub("external.sanet_relocal_demo.relocal.vlad_encoder", VLADEncoder=anything)
    _stub("external.sanet_relocal_demo.relocal_data.seven_scene.seven_scene_manual_dataset", SevenSceneManualDataset=anything)
    _stub("niantic.datasets.dataset_arparse", add_arguments_dataset=None)
    _stub("niantic.datasets.graph_structure", GraphStructure=anything)
    _stub("niantic.datasets.seven_scenes", SevenScenes=anything)
    _stub("path_config", PATH_PROJECT="")
    path = os.path.join(ref_root, "python", "niantic", "datasets", "dataset_7Scenes_multi.py")
    spec = importlib.util.spec_from_file_location("ref_dataset_7scenes_multi", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    # what is not the rule hands through
    mod.SevenSceneManualDataset = lambda **k: None
    keys = ("frames_img", "frames_ori_img", "frames_depth", "frames_Tcw", "frames_K")
    mod.DataLoader = lambda *a, **k: [{key: _Pass() for key in keys}]
    mod.preprocess_query = lambda img, *a: (img,) + (None,) * 7
    return mod


def run_reference(mod, db, q_desc, q_index, same_set, cross, sp, seed):
    """obtain_KNNs for every query in order under np.random.seed(seed): int64 [G, K]."""
    ds = object.__new__(mod.SEVEN_SCENES_multi)
    ds.DATA_PATH, ds.scene_center, ds.rand_R = None, None, None
    ds.device = contextlib.nullcontext()
    ds.query_frames = list(range(max(M, len(q_index))))
    ds.database_feats = [db[i:i + 1] for i in range(db.shape[0])]
    ds.database_set = "train"
    ds.query_set = "train" if same_set else "test"
    ds.cross_connect = cross
    current = {}
    ds.vlad_db = types.SimpleNamespace(forward=lambda _img: torch.from_numpy(current["q"]))
    np.random.seed(seed)
    out = []
    for g, qi in enumerate(q_index):
        current["q"] = q_desc[g:g + 1]
        idx, _ = ds.obtain_KNNs(int(qi), K=K, sampling_period=sp, scene_seq_len=SCENE_SEQ_LEN, seq="chess", num_workers=0)
        assert len(idx) == K, (g, len(idx))
        out.append(np.asarray(idx, dtype=np.int64))
    return np.stack(out)


def groups_of(config, q_index):
    """(q_group, db_group) of a configuration in the kernel's terms."""
    if config == "none":
        return None, None
    rows = np.arange(M, dtype=np.int64)
    if config == "self":
        return q_index.astype(np.int64), rows
    return q_index.astype(np.int64) // SCENE_SEQ_LEN, rows // SCENE_SEQ_LEN


def main(ref_root):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import retrieval_ref as R
    from relpose_gnn_amd.retrieval import RetrievalRule
    mod = load_reference_module(ref_root)
    rng = np.random.RandomState(1010)
    db = rng.standard_normal((M, D)).astype(np.float32)
    q = (db[rng.choice(M, G, replace=False)] + 0.7 * rng.standard_normal((G, D))).astype(np.float32)
    q_index = np.sort(rng.choice(M, G, replace=False)).astype(np.int64)
    fix = {"db": db, "q": q, "q_index": q_index, "k": np.int64(K), "scene_seq_len": np.int64(SCENE_SEQ_LEN)}
    seed = 100
    for config, same_set, cross in (("none", False, False), ("self", True, False), ("cross", True, True)):
        q_desc = q if config == "none" else db[q_index]          # a training-split query IS a database row
        qg, dg = groups_of(config, q_index)
        for sp in (5, 10):
            seed += 1
            got = run_reference(mod, db, q_desc, q_index, same_set, cross, sp, seed)
            ranks = RetrievalRule.reference(k=K, sampling_period=sp, seed=seed).ranks(
                R.n_allowed(M, qg, dg) if qg is not None else np.full(G, M), limit=M)
            mine = R.retrieve_ref(q_desc, db, ranks, qg, dg)
            assert np.array_equal(mine, got), (config, sp, mine, got)
            fix[f"{config}_sp{sp}_seed"] = np.int64(seed)
            fix[f"{config}_sp{sp}_indices"] = got
            fix[f"{config}_sp{sp}_max_rank"] = np.int64(ranks.max())
    out = os.path.join(HERE, "g10_retrieval.npz")
    np.savez_compressed(out, **fix)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
