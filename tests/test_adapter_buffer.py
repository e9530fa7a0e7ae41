"""slam_amd::detail::Buffer (include/slam_amd/buffer.hpp) under AddressSanitizer and UBSan, as a stand-alone program:
tests/cpp/adapter_buffer_test.cpp brings the six C-ABI functions the header calls as counting stubs over malloc / free and
checks growth, failure, moves and swaps; a leak, a double free or a failed check ends it with a non-zero status."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_buffer_under_host_sanitizers(tmp_path):
    exe = str(tmp_path / "adapter_buffer_test")
    # (the sanitizers' runtimes are linked into the program itself: it runs as it is, whatever else the process loads)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-Wall", "-Wextra", "-Wno-self-move", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "adapter_buffer_test.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip().endswith("ok")
    assert "adapter_buffer_test (expected line): stub" in p.stderr          # detail::warn's "<who>: <error>"
