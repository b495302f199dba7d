"""csrc/emit_fill.h on the CPU: the emitter's pass over one sample's chunk -- entropies from frequencies bit for bit, four-byte
frequencies widened, EV_HOST entries left alone, split over 1..17 callers in any order -- against a direct restatement
(tests/native/emit_fill_check.cpp); once more as a stand-alone program under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "emit_fill_check.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_host_pass_of_a_chunk_on_the_cpu(tmp_path, flags):
    exe = str(tmp_path / "emit_fill_check")
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off"] + flags + ["-o", exe, SRC], check=True)
    out = subprocess.run([exe, "300", "11"], check=True, capture_output=True, text=True).stdout
    assert out.startswith("ok 300 cases"), out
    assert int(out.split()[3]) > 300000, out
