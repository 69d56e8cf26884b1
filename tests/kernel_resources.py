"""The compiler's own resource report for one unit of csrc/, for the tests/test_*_build.py files: no GPU needed.

    kernel_resources("gicp.hip") -> {mangled kernel name: {"scratch": bytes per lane, "vgprs": n, "sgprs": n, "lds": bytes per block}}

One compile to an object file with the flags of csrc/Makefile (CXXFLAGS, ARCH = gfx950) plus
-Rpass-analysis=kernel-resource-usage; ``defs``: further -D / -m flags, as the Makefile's DEFS."""
import os
import re
import subprocess
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "point_cloud_registration_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

FIELDS = {"scratch": r"ScratchSize \[bytes/lane\]: (\d+)", "vgprs": r" VGPRs: (\d+)", "sgprs": r"TotalSGPRs: (\d+)",
          "lds": r"LDS Size \[bytes/block\]: (\d+)"}


def kernel_resources(hip_file, defs=()):
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fvisibility=hidden",
                            f"-I{REPO}/include", f"-I{CSRC}", *defs, "-Rpass-analysis=kernel-resource-usage", "-c",
                            os.path.join(CSRC, hip_file), "-o", os.path.join(tmp, "unit.o")], capture_output=True, text=True, check=True)
    usage, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
        for field, pattern in FIELDS.items():
            m = re.search(pattern, line)
            if m and name:
                usage[name][field] = int(m.group(1))
    return usage
