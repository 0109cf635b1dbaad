#!/usr/bin/env python3
"""Print the sha256 of the device-only assembly of every translation unit of a checkout.

    python tools/device_code_digests.py [CHECKOUT]      (default: this checkout)

Each unit of build.SOURCES is compiled with the library's own flags plus
``--cuda-device-only -S -fuse-cuid=none``.  Without the last flag the assembly names one
symbol, __hip_cuid_<hash>, after a hash of the unit's absolute path; with it the output
carries no trace of the path, so the digests of two checkouts compare directly.  A
refactor of host code leaves every digest unchanged.  Needs hipcc, no GPU.
"""
import hashlib
import importlib.util
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

root = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(__file__), ".."))
spec = importlib.util.spec_from_file_location("_aiy_build", os.path.join(root, "aiyagari_hark_amd", "build.py"))
build = importlib.util.module_from_spec(spec)
spec.loader.exec_module(build)


def digest(src):
    cmd = [build.hipcc(), f"--offload-arch={build.ARCH}"] + build.CFLAGS + [
        "--cuda-device-only", "-S", "-fuse-cuid=none", os.path.join(build.CSRC, src), "-o", "-"]
    return src, hashlib.sha256(subprocess.run(cmd, check=True, capture_output=True).stdout).hexdigest()


with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
    for src, d in ex.map(digest, build.SOURCES):
        print(f"{d}  {src}")
