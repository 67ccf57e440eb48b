"""The owning resource pool of the engine context (csrc/devpool.h) on the CPU: tests/host/devpool_host_test.cpp is a stand-alone program
over a fake backend that fails at every position of one acquisition sequence in turn, built here with the address and
undefined-behaviour sanitizers and run once."""
import os
import subprocess

from conftest import ROOT


def test_devpool_releases_exactly_once_under_sanitizers(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "tests", "host", "devpool_host_test.cpp")
    exe = str(tmp_path / "devpool_host_test")
    r = subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                        "-fno-sanitize-recover=undefined", "-O1", "-g", "-std=c++17", src, "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "devpool host test OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
