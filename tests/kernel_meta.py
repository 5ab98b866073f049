"""One csrc/*.hip compiled for gfx950 with the product's flags (chaorec_amd/_lib.py) and the per-kernel fields of the compiler's
own .amdgpu_metadata: what the host tests of the model kernels assert their kernel counts, scratch and spills on.  A helper
module, not a conftest.  The fields are read from the metadata alone; no instruction text is inspected here."""
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = {"scratch": "private_segment_fixed_size", "spills": "vgpr_spill_count", "sspills": "sgpr_spill_count",
          "lds": "group_segment_fixed_size"}


def compile_asm(source):
    """The gfx950 assembly listing (metadata included) the compiler leaves for chaorec_amd/csrc/<source>."""
    from chaorec_amd import _lib
    hipcc = "hipcc" if subprocess.run(["which", "hipcc"], capture_output=True).returncode == 0 else "/opt/rocm/bin/hipcc"
    flags = [f for f in _lib.HIPCC_FLAGS if f != "-shared"]
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.check_call([hipcc] + flags + ["-c", os.path.join(ROOT, "chaorec_amd", "csrc", source), "-o",
                                                 os.path.join(tmp, "x.o"), "-save-temps=obj"], stderr=subprocess.DEVNULL)
        with open(os.path.join(tmp, [f for f in os.listdir(tmp) if f.endswith("gfx950.s")][0])) as f:
            return f.read()


def kernel_metadata(text):
    """-> (kernel names, {"scratch" | "spills" | "sspills" | "lds": one int per kernel}) of a listing's .amdgpu_metadata."""
    meta = text.split(".amdgpu_metadata")[1]
    kernels = re.findall(r"\.name:\s+(_ZN7chaorec\w+)", meta)
    return kernels, {k: [int(x) for x in re.findall(r"\.%s:\s+(\d+)" % f, meta)] for k, f in FIELDS.items()}
