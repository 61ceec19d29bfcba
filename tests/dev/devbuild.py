"""Compile tests/dev/devcheck (the stand-alone device checker) for gfx950.

build() in __graft_entry__.py makes the binary through the csrc Makefile's
devcheck target; this rebuilds it when it is missing or older than its source
or any device header (cometbft_amd/csrc/*.h). hipcc cross-compiles, so no GPU
is needed. The binary is written beside the target and renamed over it, so a
concurrent pytest-xdist worker never executes a half-written file (ETXTBSY)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SRC = os.path.join(ROOT, "tests", "dev", "devcheck.hip")
BIN = os.path.join(ROOT, "tests", "dev", "devcheck")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def build(src=SRC, binary=BIN, flags=()):
    hdr = os.path.join(ROOT, "cometbft_amd", "csrc")
    deps = [src] + [os.path.join(hdr, f) for f in os.listdir(hdr) if f.endswith(".h")]
    if not os.path.exists(binary) or os.path.getmtime(binary) < max(os.path.getmtime(d) for d in deps):
        tmp = f"{binary}.{os.getpid()}"
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-function"] + list(flags)
                       + ["-o", tmp, src], check=True)
        os.replace(tmp, binary)
    return binary
