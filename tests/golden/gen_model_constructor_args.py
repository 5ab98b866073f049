#!/usr/bin/env python
"""Generate tests/golden/model_constructor_args.json: what main.build_model hands every model's constructor.

Every model class is replaced by a recorder for the duration of the run; build_model is called for each name with
parse_args(["--Model", name, "--data_path", "sports", "--data_root", DATA_ROOT]) plus the first point of the name's YAML grid,
sentinel strings for the data arguments, num_user = 11 and num_item = 7.  Stored per name: [class name, positional arguments,
keyword arguments, class attributes set].  No GPU, no data file.  The committed file was written by this script at the commit
BEFORE the constructor table moved into chaorec_amd/registry.py; tests/test_model_registry.py replays record() against the
registry and compares exactly.

    python tests/golden/gen_model_constructor_args.py
"""
import inspect
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "model_constructor_args.json")
DATA_ROOT = "DATA_ROOT"
NUM_USER, NUM_ITEM = 11, 7
SENTINELS = ("train_data", "user_item_dict", "v_feat", "t_feat", "device")


def _names():
    """Model_YAML/*.yaml: one file per --Model name."""
    import chaorec_amd
    folder = os.path.join(os.path.dirname(chaorec_amd.__file__), "Model_YAML")
    return sorted(f[:-5] for f in os.listdir(folder) if f.endswith(".yaml"))


def _swap_classes():
    """Replace every class Model/__init__.py exports by a recorder class of the same name, in every chaorec_amd module that
    holds it.  Returns (calls, undo): calls receives (recorder class, args, kwargs) per construction."""
    import chaorec_amd.main  # noqa: F401  (and, through it, every module that holds the classes)
    from chaorec_amd import Model
    calls, undo = [], []
    for cname, cls in [(n, c) for n, c in vars(Model).items() if inspect.isclass(c)]:
        def __init__(self, *args, **kwargs):
            calls.append((type(self), list(args), kwargs))
        rec = type(cname, (), {"__init__": __init__})
        for mod in [m for n, m in sys.modules.items() if n.startswith("chaorec_amd") and m is not None]:
            for attr, value in list(vars(mod).items()):
                if value is cls:
                    undo.append((mod, attr, cls))
                    setattr(mod, attr, rec)
    return calls, undo


def record():
    """name -> [class name, positional args, keyword args, class attributes set] for every --Model name."""
    from chaorec_amd.arg_parser import load_yaml_config, parse_args
    from chaorec_amd.main import build_model
    out = {}
    for name in _names():
        calls, undo = _swap_classes()
        try:
            args = parse_args(["--Model", name, "--data_path", "sports", "--data_root", DATA_ROOT])
            cfg = load_yaml_config(name)
            for p in cfg["hyper_parameters"]:
                setattr(args, p, cfg[p][0])
            build_model(args, NUM_USER, NUM_ITEM, *SENTINELS)
            (cls, pos, kw), = calls
            # every recorder class of this round: the path attributes are set on a class, not on the instance
            set_attrs = {}
            for mod, attr, _ in undo:
                rec = getattr(mod, attr)
                set_attrs.update({f"{rec.__name__}.{k}": v for k, v in vars(rec).items() if not k.startswith("__")})
            out[name] = [cls.__name__, pos, kw, set_attrs]
        finally:
            for mod, attr, cls in undo:
                setattr(mod, attr, cls)
    return json.loads(json.dumps(out))          # (tuples become lists here as they do in the file)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    with open(FIXTURE, "w") as f:
        json.dump(record(), f, indent=0, sort_keys=True)
        f.write("\n")
    print(FIXTURE, os.path.getsize(FIXTURE), "bytes")
