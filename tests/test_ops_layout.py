"""The Python-to-C boundary's layout: one wrapper module per kernel family, every public name of theirs reachable as
chaorec_amd.ops.<name> (derived from the modules' __all__, no list kept by hand) and as chaorec_amd.ops_extra.<name> (a
compatibility module that defines nothing).  tests/golden/ops_names.txt holds the (route, name) pairs that resolved before the
split: names only."""
import ast
import importlib
import inspect
import os

import pytest
import torch

from chaorec_amd import ops, ops_extra
from conftest import GOLDEN, ROOT

FAMILIES = [importlib.import_module("chaorec_amd." + m) for m in ops._FAMILY_MODULES]
EXTRA_FAMILIES = [m for m in FAMILIES if m.__name__ != "chaorec_amd.ops_dense"]     # ops_extra never held the dense products


def test_recorded_names_resolve():
    with open(os.path.join(GOLDEN, "ops_names.txt")) as f:
        pairs = [line.split() for line in f if line.strip()]
    assert sum(route == "ops_extra" for route, _ in pairs) == 147 and len(pairs) == 147 + 95
    routes = {"ops": ops, "ops_extra": ops_extra}
    missing = [(route, name) for route, name in pairs if not hasattr(routes[route], name)]
    assert not missing, missing


def test_both_routes_give_the_family_modules_objects():
    assert ops._FAMILY_MODULES[0] == "ops_dense"
    for m in FAMILIES:
        for name in m.__all__:
            assert getattr(ops, name) is getattr(m, name), (m.__name__, name)
            assert ops.__dict__[name] is getattr(m, name), f"ops.{name} is not cached after its first lookup"
    for m in EXTRA_FAMILIES:
        for name in m.__all__:
            assert getattr(ops_extra, name) is getattr(m, name), (m.__name__, name)
    assert set().union(*(m.__all__ for m in FAMILIES)) <= set(dir(ops))


def test_family_all_lists_are_disjoint_and_complete():
    seen = {}
    for m in FAMILIES:
        assert len(set(m.__all__)) == len(m.__all__), m.__name__
        for name in m.__all__:
            assert hasattr(m, name), (m.__name__, name)
            assert name not in seen, f"{name} in {seen.get(name)} and {m.__name__}"
            seen[name] = m.__name__
        defined = {n for n, v in vars(m).items()
                   if (inspect.isfunction(v) or inspect.isclass(v)) and v.__module__ == m.__name__ and v.__name__ != "<lambda>"}
        assert defined <= set(m.__all__), (m.__name__, sorted(defined - set(m.__all__)))


def test_only_listed_names_resolve_through_ops():
    with pytest.raises(AttributeError, match="torch_nonexistent_xyz"):
        getattr(ops, "torch_nonexistent_xyz")
    # what a family module merely imports (`_ops`, `_os`, ...) does not leak through the facade, unless ops.py has that name itself
    listed = set().union(*(m.__all__ for m in FAMILIES))
    leaks = {n for m in FAMILIES for n in vars(m) if not n.startswith("__") and n not in listed and n not in vars(ops)}
    assert "_ops" in leaks
    for name in sorted(leaks):
        with pytest.raises(AttributeError):
            getattr(ops, name)
    assert ops.ctypes is importlib.import_module("ctypes") and ops.torch is torch       # ops.py imports these itself


def test_ops_extra_defines_nothing():
    with open(os.path.join(ROOT, "chaorec_amd", "ops_extra.py")) as f:
        tree = ast.parse(f.read())
    bad = [n.lineno for n in ast.walk(tree) if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef, ast.Lambda))]
    assert not bad, bad


def test_typed_messages():
    x = torch.zeros(2, 3, dtype=torch.float64)
    with pytest.raises(ValueError) as e:
        ops._typed("model", x, "x", torch.float32)
    assert str(e.value) == "model: x must be a contiguous float32 tensor"
    with pytest.raises(ValueError) as e:
        ops._f32("model", x, "x")
    assert str(e.value) == "model: x must be a contiguous float32 tensor"
    with pytest.raises(ValueError) as e:
        ops._i32("usergraph", x, "col")
    assert str(e.value) == "usergraph: col must be a contiguous int32 tensor"
    with pytest.raises(ValueError) as e:
        ops._f32("model", torch.zeros(3, 2).t(), "x")            # right dtype, not contiguous
    assert str(e.value) == "model: x must be a contiguous float32 tensor"
    y = torch.zeros(2, 3)
    with pytest.raises(ValueError) as e:
        ops._f32("model", y, "y", (3, 2))
    assert str(e.value) == "model: y is (2, 3), expected (3, 2)"
    assert ops._f32("model", y, "y", (2, 3)) is y and ops._i32("m", y.int(), "y").dtype == torch.int32
    # the old names keep the old signatures
    assert ops_extra._vae_f32("model", y, "y") is y
    with pytest.raises(ValueError) as e:
        ops_extra._ug_i32(y, "nbr_idx", (2, 3))
    assert str(e.value) == "usergraph: nbr_idx must be a contiguous int32 tensor"
    with pytest.raises(ValueError) as e:
        ops._check_dim("MHRec", 32, 64)
    assert str(e.value) == "MHRec: dim_E=32; the kernels tile D=64"
    assert ops._empty_f32("cpu")(2, 3).shape == (2, 3) and ops._empty_f32("cpu")(1).dtype == torch.float32
    assert ops.macrid_topk is ops.rows_topk
