"""Builds tests/cpp/normal_cdf_test.cpp -- ml_amd/csrc/device/normal_cdf.hpp included as plain host code, in a program with its own
main -- with g++ -fsanitize=address,undefined,float-cast-overflow and runs it: special values, no step down over a dense grid, the library's erfc as a
second opinion, the quantile's round trip and oddness. The sanitizers see the stand-alone program only. Where the environment already
preloads a library into every process (tests/test_sanitizers.py runs the suite that way), a second sanitizer runtime cannot start
beside it: the program is then built plain, as normal_cdf_test_plain, and the environment is left as it is."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "normal_cdf_test.cpp")
HEADERS = os.path.join(ROOT, "ml_amd", "csrc", "device")
EXE = os.path.join(ROOT, "tests", "cpp", "normal_cdf_test")
SANITIZE = ["-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=undefined,float-cast-overflow"]


def test_normal_cdf_as_a_sanitized_host_program():
    deps = [SRC, os.path.join(HEADERS, "normal_cdf.hpp"), os.path.join(HEADERS, "exp_nonpos.hpp")]
    plain = bool(os.environ.get("LD_PRELOAD"))
    exe = EXE + "_plain" if plain else EXE
    if not os.path.exists(exe) or os.path.getmtime(exe) <= max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra"] + ([] if plain else SANITIZE) +
                              ["-I", HEADERS, SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
