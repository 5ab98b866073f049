"""chaorec_amd/registry.py: the one table behind main, the training loop and the tools.  No GPU.

The expected traits below are literals: the name tuples main.py and train_and_evaluate.py held before the table existed
(needs_feat, MMGCN_STYLE, PRE_EPOCH, E_STEP, BUILD_FIRST, NO_CAPTURE, the `if model_name ==` chain of train(), the BSPM branch,
the ('BSPM', 'CF_Diff') optimizer tuple).  The constructor arguments are a record taken at that commit
(tests/golden/gen_model_constructor_args.py), replayed here against the table."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from chaorec_amd import Model, dataload, epochs, main, registry, train_and_evaluate as te
from chaorec_amd.arg_parser import parse_args
from chaorec_amd.registry import MODELS, ModelSpec, spec_of

HERE = os.path.dirname(os.path.abspath(__file__))

FEATURES = {"MMGCN", "FREEDOM", "MGCN", "VBPR", "SLMRec", "MCLN", "POWERec", "LGMRec", "SMORE", "MMGCL", "LightGT", "GUME", "DDRec", "MICRO",
            "MENTOR", "BM3", "MGCL", "LATTICE", "MMSSL", "GRCN", "MGAT", "DRAGON", "DualGNN", "COHESION", "MVGAE", "DiffMM", "Grade", "MHRec"}
PRE_EPOCH = {"FREEDOM", "LayerGCN", "POWERec", "DRAGON", "DualGNN", "COHESION"}
BEFORE_STEP = {"NCL", "VGCL"}
BUILD_FIRST = {"LATTICE", "MICRO"}
NO_CAPTURE = {"NCL", "VGCL", "LATTICE", "MICRO", "SGL", "SelfCF", "MMGCL", "LightGT", "MMSSL", "DiffMM", "AdaGCL", "GraphAug", "Grade", "MHRec",
              "CF_Diff"}
PAIRS = {"MMGCN", "GRCN"}
EPOCH = {"MHRec": epochs._train_epoch_mhrec, "MMSSL": epochs._train_epoch_mmssl, "DiffMM": epochs._train_epoch_diffmm,
         "CF_Diff": epochs._train_epoch_cfdiff, "AdaGCL": epochs._train_epoch_adagcl, "Grade": epochs._train_epoch_grade}
UNKNOWN = "NoSuchModel"


def names_where(pred):
    return {name for name, spec in MODELS.items() if pred(spec)}


def test_traits_are_the_parent_commit_s():
    assert (len(FEATURES), len(PRE_EPOCH), len(NO_CAPTURE), len(MODELS)) == (28, 6, 15, 51)
    assert names_where(lambda s: s.features) == FEATURES
    assert names_where(lambda s: s.pre_epoch) == PRE_EPOCH
    assert names_where(lambda s: s.before_step is not None) == BEFORE_STEP
    assert names_where(lambda s: s.build_first) == BUILD_FIRST
    assert names_where(lambda s: not s.capture) == NO_CAPTURE
    assert names_where(lambda s: s.batch == "pairs") == PAIRS
    assert {name: spec.epoch for name, spec in MODELS.items() if spec.epoch is not None} == EPOCH
    assert names_where(lambda s: not s.trains) == {"BSPM"}
    assert names_where(lambda s: not s.main_optimizer) == {"BSPM", "CF_Diff"}
    assert all(callable(spec.build) for spec in MODELS.values())
    with pytest.raises(Exception):                       # frozen
        MODELS["LightGCN"].capture = False


def test_names_are_the_exported_classes_and_the_yaml_files():
    classes = {name for name, value in vars(Model).items() if isinstance(value, type)}
    assert len(classes) == 51 and {"BPR" if c == "BPRMF" else c for c in classes} == set(MODELS)
    yamls = {f[:-5] for f in os.listdir(os.path.join(os.path.dirname(main.__file__), "Model_YAML")) if f.endswith(".yaml")}
    assert yamls == set(MODELS)


def test_constructor_arguments_are_the_parent_commit_s():
    spec = importlib.util.spec_from_file_location("gen_model_constructor_args", os.path.join(HERE, "golden", "gen_model_constructor_args.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(gen.FIXTURE) as f:
        want = json.load(f)
    before = {name: value for name, value in vars(Model).items() if isinstance(value, type)}
    got = gen.record()
    assert {name: value for name, value in vars(Model).items() if isinstance(value, type)} == before     # the recorders are gone again
    assert list(got) == list(want) and len(want) == 51
    for name in want:
        assert got[name] == want[name], name
    paths = {name: rec[3] for name, rec in want.items() if rec[3]}
    graph = "DATA_ROOT/sports/user_graph_dict.npy"
    assert paths == {"MHRec": {"MHRec.data_dir": "DATA_ROOT/sports"}, "COHESION": {"COHESION.user_graph_path": graph},
                     "DualGNN": {"DualGNN.user_graph_path": graph}, "DRAGON": {"DRAGON.user_graph_path": graph}}
    assert want["CF_Diff"][:3] == ["CF_Diff", [11, 7, "user_item_dict", 0.1, 0.0005, 0.005, 10, 0.001, "device"], {"seed": 42}]


@pytest.mark.parametrize("name", list(MODELS))
def test_batch_is_what_the_host_sampler_returns(name):
    U, I = 3, 4
    edges = np.array([[0, 3], [0, 4], [1, 5], [2, 6], [2, 3]])
    uid = {0: [3, 4], 1: [5], 2: [6, 3]}
    item = dataload.TrainingDataset(U, I, uid, edges, name)[0]
    batch = MODELS[name].batch
    if batch == "triple":
        assert len(item) == 3 and all(type(x) is int for x in item)
    elif batch == "pairs":
        assert len(item) == 2 and all(isinstance(x, torch.LongTensor) and x.shape == (2,) for x in item)
    elif batch == "second_negative":
        assert name == "MCLN" and len(item) == 4 and all(type(x) is int for x in item)
    else:
        assert batch == "sequences" and name == "LightGT" and len(item) == 4
        assert all(isinstance(x, torch.LongTensor) and x.shape == (2,) for x in item[:2])
        assert item[2].dtype == torch.bool and item[3].dtype == torch.int64 and item[2].shape == item[3].shape == (51,)


def test_one_model_each_for_the_two_special_batches():
    assert names_where(lambda s: s.batch == "sequences") == {"LightGT"} and names_where(lambda s: s.batch == "second_negative") == {"MCLN"}
    assert {spec.batch for spec in MODELS.values()} == {"triple", "pairs", "second_negative", "sequences"}


class StandIn(torch.nn.Module):
    """loss(x) = w * x; records what ran, in order."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(()))
        self.calls = []

    def loss(self, x, build_item_graph=None):
        self.calls.append(("loss", float(self.w.detach()), build_item_graph))
        return self.w * x


def test_an_unknown_name_takes_the_generic_loop():
    assert UNKNOWN not in MODELS and spec_of(UNKNOWN) == ModelSpec(build=None) and spec_of("Grade") is MODELS["Grade"]
    m = StandIn()
    total = te.train(m, [(torch.tensor(2.0),)] * 2, torch.optim.SGD(m.parameters(), lr=0.25), UNKNOWN)
    # two steps: w = 1 then 1 - 0.25 * 2 = 0.5; the summed loss 2 + 1
    assert m.calls == [("loss", 1.0, None), ("loss", 0.5, None)] and total == 3.0 and float(m.w.detach()) == 0.0
    assert te._capture_step(m, [(torch.tensor(2.0),)] * 2, None, UNKNOWN) is None
    args = parse_args(["--Model", "LightGCN"])
    args.Model = UNKNOWN
    with pytest.raises(SystemExit) as exc:
        main.build_model(args, 11, 7, None, None, None, None, "cpu")
    assert str(exc.value) == f"--Model {UNKNOWN}: only {sorted(MODELS)} are on the MI355X hot path"


def test_train_hands_the_epoch_of_the_entry_its_three_arguments(monkeypatch):
    seen = []
    monkeypatch.setitem(registry.MODELS, UNKNOWN, ModelSpec(build=None, epoch=lambda *a: seen.append(a) or 7.5))
    m, loader, opt = StandIn(), [(torch.tensor(2.0),)], object()
    assert te.train(m, loader, opt, UNKNOWN) == 7.5 and m.training
    assert len(seen) == 1 and len(seen[0]) == 3 and seen[0][0] is m and seen[0][1] is loader and seen[0][2] is opt
    assert m.calls == []


def test_before_step_runs_once_per_batch_before_loss(monkeypatch):
    monkeypatch.setitem(registry.MODELS, UNKNOWN, ModelSpec(build=None, before_step=lambda model: model.calls.append("before")))
    m = StandIn()
    te.train(m, [(torch.tensor(2.0),)] * 3, torch.optim.SGD(m.parameters(), lr=0.25), UNKNOWN)
    assert [c if c == "before" else c[0] for c in m.calls] == ["before", "loss"] * 3


def test_the_entries_before_step_call_what_the_reference_s_loop_calls():
    class Clustering:
        def __init__(self):
            self.calls = []

        def forward(self):
            self.calls.append("forward")

        def e_step(self):
            self.calls.append("e_step")
    ncl, vgcl = Clustering(), Clustering()
    MODELS["NCL"].before_step(ncl)
    MODELS["VGCL"].before_step(vgcl)
    assert ncl.calls == ["e_step"] and vgcl.calls == ["forward", "e_step"]


def test_build_first_passes_true_then_false(monkeypatch):
    monkeypatch.setitem(registry.MODELS, UNKNOWN, ModelSpec(build=None, build_first=True))
    m = StandIn()
    te.train(m, [(torch.tensor(2.0),)] * 3, torch.optim.SGD(m.parameters(), lr=0.25), UNKNOWN)
    assert [c[2] for c in m.calls] == [True, False, False]
