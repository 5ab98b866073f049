"""ctypes binding of libchaorec_hip.so (include/chaorec_hip.h).

The HIP library IS the product's compute path: there is no CPU or eager-PyTorch fallback.
`load()` raises if the shared object is missing, and every op in chaorec_amd.ops raises on
non-CUDA tensors.

The header is the only description of the ABI: SIGNATURES and ABI_VERSION are parsed from it at import, and `load()`
makes every export that returns a status raise on a non-zero one.  Adding an export = its prototype in the header, its
kernel, and its wrapper in ops*.py; nothing here changes (but INT_VALUE_EXPORTS, if its `int` result is a value).
"""
import ctypes
import os
import re
import shutil
import subprocess

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
LIB_PATH = os.path.join(_CSRC, "libchaorec_hip.so")
SOURCES = ["spmm.hip", "spmm_fewsrc.hip", "bpr.hip", "bpr_frontier.hip", "score_topk.hip", "topk_wide.hip", "gemm.hip", "gemm_bf16x3.hip", "metrics.hip", "graph_dropout.hip",
           "rowops.hip", "feature_adam.hip", "exchange.hip", "dgcf.hip", "multvae.hip", "macridvae.hip",
           "dualvae.hip", "usergraph.hip", "mvgae.hip", "diffmm.hip", "graphaug.hip", "mhrec.hip", "grade.hip", "cfdiff.hip", "diffrec.hip", "lightgode.hip", "bspm.hip", "adagcl.hip"]
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off",
               "-mllvm", "-amdgpu-mfma-vgpr-form"]   # MFMA results in VGPRs: no v_accvgpr_read per compared score

_lib = None
_HEADER = os.path.join(os.path.dirname(_CSRC), "..", "include", "chaorec_hip.h")
_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32,
            "uint64_t": ctypes.c_uint64, "float": ctypes.c_float, "size_t": ctypes.c_size_t}
# exports whose `int` result the caller reads; every other `int` result is a status that load() checks
INT_VALUE_EXPORTS = {"chaorec_abi_version", "chaorec_spmm_rows_per_wave", "chaorec_spmm_long_threshold",
                     "chaorec_adam_lowrank_strips", "chaorec_adam_multi_max",
                     "chaorec_dgcf_check_shape"}   # a status, turned into a ValueError by ops_dgcf.dgcf_check_shape


def _ctype(decl, name, is_return=False):
    """One return type or one parameter (its name optional) -> the ctypes type; never a guess."""
    words = decl.replace("*", " * ").split()
    if re.search(r"[^\w\s*]", decl):      # an array, a function pointer, `...`: not this header's style
        words = []
    if "*" in words:
        if not is_return:
            return ctypes.c_void_p
        if words == ["const", "char", "*"]:
            return ctypes.c_char_p
    elif words and words[0] in _SCALARS and len(words) <= (1 if is_return else 2):
        return _SCALARS[words[0]]
    raise ValueError(f"chaorec_hip.h: {name}: no ctypes type for '{decl.strip()}'")


def parse_header(text):
    """(ABI version, {name: (restype, [argtypes])}) of a header in chaorec_hip.h's plain style: comments, preprocessor
    lines and the extern "C" braces aside, it is nothing but `type chaorec_name(type [name], ...);` prototypes."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    version = re.search(r"^[ \t]*#[ \t]*define[ \t]+CHAOREC_ABI_VERSION[ \t]+(\d+)[ \t]*$", text, flags=re.M)
    if not version:
        raise ValueError("chaorec_hip.h: no '#define CHAOREC_ABI_VERSION <number>'")
    text = re.sub(r'^[ \t]*#.*$|extern\s+"C"\s*\{|\}', " ", text, flags=re.M)
    sigs = {}
    for stmt in filter(None, (" ".join(s.split()) for s in text.split(";"))):
        m = re.fullmatch(r"(.+?)\b(chaorec_\w+) ?\((.*)\)", stmt)
        if not m or m.group(2) in sigs:
            raise ValueError(f"chaorec_hip.h: not the one prototype of a chaorec_* function: '{stmt}'")
        ret, name, params = m.groups()
        params = [] if params.strip() in ("", "void") else params.split(",")
        sigs[name] = (_ctype(ret, name, True), [_ctype(p, name) for p in params])
    return int(version.group(1)), sigs


if not os.path.exists(_HEADER):
    raise RuntimeError(f"{os.path.normpath(_HEADER)} is missing: the ctypes binding of libchaorec_hip.so is derived from "
                       "it (chaorec_amd ships with its include/ directory).")
with open(_HEADER) as _f:
    ABI_VERSION, SIGNATURES = parse_header(_f.read())   # name -> (restype, argtypes), applied to the CDLL by load()


def _experiment_flags():
    """(extra, dropped) hipcc flags of an experiment build (tools/*_variants.py): CHAOREC_EXTRA_HIPCC_FLAGS /
    CHAOREC_DROP_HIPCC_FLAGS (e.g. "-mllvm -amdgpu-mfma-vgpr-form")."""
    return (os.environ.get("CHAOREC_EXTRA_HIPCC_FLAGS", "").split(), os.environ.get("CHAOREC_DROP_HIPCC_FLAGS", "").split())


def _experiment_tag():
    extra, drop = _experiment_flags()
    if not extra and not drop:
        return ""
    import hashlib
    return hashlib.sha1((" ".join(extra) + "|" + " ".join(drop)).encode()).hexdigest()[:10]


def current_lib_path():
    """The product library -- or, only while an experiment's flags are in the environment, that experiment's own file."""
    tag = _experiment_tag()
    return os.path.join(_CSRC, "exp", f"libchaorec_hip_{tag}.so") if tag else LIB_PATH


def build(force=False, verbose=False):
    """Cross-compile the HIP kernels for gfx950 into csrc/libchaorec_hip.so (no GPU needed): one object per source
    file (compiled in parallel, re-compiled only when the file or a header changed), then one link."""
    from concurrent.futures import ThreadPoolExecutor
    srcs = [os.path.join(_CSRC, s) for s in SOURCES]
    hdrs = [os.path.join(_CSRC, f) for f in sorted(os.listdir(_CSRC)) if f.endswith((".h", ".hpp"))]
    hdrs += [_HEADER, os.path.abspath(__file__)]
    extra, drop = _experiment_flags()
    lib_path = current_lib_path()
    if not force and os.path.exists(lib_path) and all(os.path.getmtime(lib_path) >= os.path.getmtime(d) for d in srcs + hdrs):
        return lib_path
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    # an experiment build (extra / dropped compiler flags) has its own objects and its own library: it can never
    # replace, or be mistaken for, the product build
    tag = _experiment_tag()
    objdir = os.path.join(_CSRC, "build" + (("_exp_" + tag) if tag else ""))
    os.makedirs(objdir, exist_ok=True)
    os.makedirs(os.path.dirname(lib_path), exist_ok=True)
    cflags = [f for f in HIPCC_FLAGS if f != "-shared" and f not in drop] + extra

    def compile_one(src):
        obj = os.path.join(objdir, os.path.basename(src) + ".o")
        if (not force and os.path.exists(obj)
                and all(os.path.getmtime(obj) >= os.path.getmtime(d) for d in [src] + hdrs)):
            return obj
        cmd = [hipcc] + cflags + ["-c", src, "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
        return obj

    with ThreadPoolExecutor(max_workers=min(len(srcs), os.cpu_count() or 4)) as ex:
        objs = list(ex.map(compile_one, srcs))
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib_path] + objs
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return lib_path


def ensure_built():
    """Entry points that own a whole run (bench.py, smoke(), the test session) call this first: compile the library
    if the file is not there (a fresh checkout; hipcc cross-compiles without a GPU).  load() itself never builds and
    never falls back: a missing library is an error for every op."""
    if not os.path.exists(current_lib_path()):
        build(verbose=True)
    return current_lib_path()


def load():
    global _lib
    if _lib is not None:
        return _lib
    lib_path = current_lib_path()
    if not os.path.exists(lib_path):
        raise RuntimeError(
            f"{lib_path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or chaorec_amd._lib.build()).  chaorec_amd has no CPU fallback.")
    # torch first: it brings its own HIP runtime (libamdhip64 of its ROCm build); a process in which THIS library pulled
    # in the system's copy before torch was imported ended with "no ROCm-capable device is detected" at the first launch
    # (python __graft_entry__.py smoke: build() loads the library, smoke() then imported torch)
    import torch  # noqa: F401
    lib = ctypes.CDLL(lib_path)
    def raise_on_status(rc, fn, args):
        if rc != 0:
            msg = lib.chaorec_last_error()
            raise RuntimeError(f"{fn.__name__} failed ({rc}): {msg.decode() if msg else ''}")
        return rc

    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError here = header/library drift
        fn.restype = res
        fn.argtypes = args
        if res is ctypes.c_int and name not in INT_VALUE_EXPORTS:
            fn.errcheck = raise_on_status   # a status is checked here, under the called function's own name
    if lib.chaorec_abi_version() != ABI_VERSION:
        raise RuntimeError("libchaorec_hip.so ABI version mismatch")
    _lib = lib
    return lib
