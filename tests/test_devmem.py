"""The owning device / pinned buffer types (sentinel_amd/csrc/devmem.h) over counting stub allocators, built with
ASan + UBSan as a stand-alone program (tests/cpp/test_devmem_host.cpp): move leaves the source empty, a failed
reserve leaves nullptr and 0, reserve within the size does not reallocate, every allocation is freed exactly once."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_devmem_over_counting_allocators(tmp_path):
    exe = tmp_path / "tdm"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", str(exe),
                           os.path.join(ROOT, "tests/cpp/test_devmem_host.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    assert out.stdout.startswith("OK")
