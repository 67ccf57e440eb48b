"""The env-group worker's hand-off (csrc/group_worker.h: post / drain / sleep and wake / stop, the rc / err hand-back) on the CPU:
tests/host/group_worker_host_test.cpp is a stand-alone program whose jobs write into an array, built here once with the thread
sanitizer and once with the address and undefined-behaviour sanitizers, and run once each."""
import os
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.parametrize("sanitize", ["thread", "address,undefined"])
def test_group_worker_hand_off_under_sanitizers(tmp_path, sanitize):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "tests", "host", "group_worker_host_test.cpp")
    exe = str(tmp_path / "group_worker_host_test")
    r = subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=" + sanitize, "-Xarch_host",
                        "-fno-sanitize-recover=undefined", "-O1", "-g", "-std=c++17", "-pthread", src, "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "group worker host test OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
