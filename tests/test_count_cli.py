"""dsm_count without a GPU: usage errors exit 1 with the usage line before any HIP call, and the batched pattern reader of
csrc/count_input.h against a direct restatement (tests/native/count_input_check.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "dsm-framework_amd", "host", "dsm_count")


def test_usage_errors_exit_1_with_the_usage_line(tmp_path):
    assert os.path.exists(EXE), "host/dsm_count is not built"
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")  # (a HIP call would fail differently; none is made)
    for args in ([], ["--bogus", "a.fmi"], ["-x", "a.fmi"], ["-f"], ["-f", "two", "a.fmi"], ["-f", "-1", "a.fmi"], ["-k", "13", "a.fmi"],
                 ["--device", "x", "a.fmi"], ["--all", "-f", "3"]):
        r = subprocess.run([EXE] + args, input=b"ACGT\n", capture_output=True, timeout=60, env=env, cwd=str(tmp_path))
        assert r.returncode == 1, (args, r.returncode, r.stderr)
        assert r.stderr.decode().splitlines()[0].startswith("usage: dsm_count "), (args, r.stderr)
        assert r.stdout == b"", args


def test_count_input_reader_native(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("native") / "count_input_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "native", "count_input_check.cpp")], check=True)
    for seed in (1, 2):
        r = subprocess.run([exe, "3000", str(seed)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert "count_input ok" in r.stdout
