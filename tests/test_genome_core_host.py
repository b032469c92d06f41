"""CPU: the per-line rules of the organism-file parser (metalign_amd/csrc/mg_genome_core.h) compiled for the host
(tests/host_genome_check.cpp) against the definition, build_db.genome_bases, on the cases of tests/genome_cases.py — once as
built, once under the address and undefined-behaviour sanitizers.  No GPU needed."""
import os
import struct
import subprocess

import pytest

import genome_cases as gc

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_genome_check.cpp")


def build(out, extra=()):
    subprocess.check_call(["g++", "-O1", "-std=c++20", "-Wall", *extra, "-o", out, SRC])
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build(str(tmp_path_factory.mktemp("genome") / "host_genome_check"))


@pytest.fixture(scope="module")
def exe_sanitized(tmp_path_factory):
    d = tmp_path_factory.mktemp("genome_san")
    probe = d / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]
    if subprocess.run(["g++", *flags, "-o", str(d / "probe"), str(probe)], capture_output=True).returncode != 0:
        return None  # (this compiler does not link those runtimes: the plain build above is the check)
    return build(str(d / "host_genome_check_san"), flags)


@pytest.fixture(scope="module")
def wanted(tmp_path_factory):
    gc.self_check()
    return {name: gc.expected(files, tmp_path_factory.mktemp("want_" + name)) for name, files in gc.CASES.items()}


def run(exe, files, tmp_path):
    p = tmp_path / "cases.bin"
    p.write_bytes(struct.pack("<I", len(files)) + b"".join(struct.pack("<I", len(f)) + f for f in files))
    out = subprocess.run([exe, str(p)], capture_output=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    got = []
    for ln in out.stdout.decode().splitlines():
        got.append(None if ln == "undecided" else bytes.fromhex(ln.split(" ", 1)[1] if " " in ln else ""))
    return got


@pytest.mark.parametrize("name", sorted(gc.CASES))
def test_core_header_is_genome_bases(exe, wanted, tmp_path, name):
    assert run(exe, gc.CASES[name], tmp_path) == wanted[name]


def test_core_header_under_sanitizers(exe_sanitized, wanted, tmp_path):
    if exe_sanitized is None:
        pytest.skip("this compiler does not link the address / undefined-behaviour sanitizer runtimes")
    for name, files in gc.CASES.items():
        assert run(exe_sanitized, files, tmp_path) == wanted[name], name


def test_all_cases_in_one_buffer(exe, wanted, tmp_path):
    files = [f for name in sorted(gc.CASES) for f in gc.CASES[name]]
    assert run(exe, files, tmp_path) == [w for name in sorted(gc.CASES) for w in wanted[name]]
